"""The reverse-mode gradient of the forward dynamics on the GPU (multibody_fd_vjp_batch_* /
multibody_fd_vjp_plain_batch_*, fd_vjp_body.hip.hpp) and its torch.autograd wrapper.  B = 257: one full
256-lane block plus a one-lane tail; fp64 runs on rows of leading dimension B + 3.  The five models cover
both forms of the forward stage (FR3 and the 12-link general-axes chain: the mass-matrix form; 16 links,
the tree and the floating base: the ABA) and every Topo branch.  Reference: tests/fd_vjp_ref.py; bounds
are the header's contracts."""
import re

import numpy as np
import pytest
import torch

import fd_vjp_ref as fv

pytestmark = pytest.mark.gpu

B, NREF = 257, 40
MODELS = ["fr3", "general12", "chain16", "tree9", "floating14"]
DEV = "cuda:0"
_CACHE = {}

# Measured on the MI355X (B = 257), and the bounds made of them.
# Against the composition: g_qd and g_fext are bit for bit the composition's on all five models; g_q differs in
# the last bit (2.856e-16 scaled at most, 12 links with general axes; FR3 1.19e-16, 16 links 2.42e-16, the tree
# 2.31e-16, floating base 1.13e-16): this kernel is built with the forward dynamics' centre-of-mass link forces
# (so that its qdd is fd_ext's, which held bit for bit), rnea_vjp's own kernel with the origin form.  10x.
COMPOSITION_BOUND = 2.86e-15
# Kernel against the host form of the same lane body: 2.528e-14 (FR3; 16 links 1.80e-14).  10x.
HOST_FORM_BOUND = 2.53e-13
# fp32 against the fp64 kernel: 2.224e-5 (FR3; the tree 1.75e-6, floating base 5.50e-6).  About 7x.
F32_BOUND = 1.6e-4


@pytest.fixture(scope="module")
def ffi():
    from rigidbody_amd import ffi

    if not hasattr(ffi.Multibody, "fd_vjp_batch"):
        pytest.fail("the binding has no fd_vjp entry points")
    return ffi


def _rows(x, dtype=torch.float64, pad=3):
    """[rows, B] on the device, on rows of leading dimension B + pad."""
    t = torch.empty((x.shape[0], x.shape[1] + pad), dtype=dtype, device=DEV)[:, :x.shape[1]]
    t.copy_(torch.as_tensor(x))
    return t


def _case(case):
    """Model, host inputs, device inputs and both kernels' fp64 outputs (device tensors and numpy), computed
    once: (qdd, g_q, g_qd, g_tau[, g_fext])."""
    if case not in _CACHE:
        mb, om, m6 = fv.setup(case)
        q, qd, _, tau, fext = fv.inputs(mb, B, 91)
        w = fv.cotangent(mb, B, 92)
        host = dict(q=q, qd=qd, tau=tau, fext=fext, w=w)
        dev = {k: _rows(v) for k, v in host.items()}
        t_ext = mb.fd_vjp_batch(dev["q"], dev["qd"], dev["tau"], dev["w"], fext=dev["fext"])
        t_pl = mb.fd_vjp_batch(dev["q"], dev["qd"], dev["tau"], dev["w"])
        assert len(t_ext) == 5 and len(t_pl) == 4
        _CACHE[case] = (mb, om, m6, host, dev, t_ext, t_pl, [t.cpu().numpy() for t in t_ext],
                        [t.cpu().numpy() for t in t_pl])
    return _CACHE[case]


@pytest.mark.parametrize("case,ext", [(c, True) for c in MODELS] + [("fr3", False), ("floating14", False)])
def test_reference_parity_f64(ffi, case, ext):
    mb, om, m6, h, _, _, _, g_ext, g_pl = _case(case)
    d = fv.direction(mb, NREF, 93, ext)
    s = slice(0, NREF)
    ref, err = fv.directional(om, m6, h["q"][:, s], h["qd"][:, s], h["tau"][:, s], h["fext"][:, s] if ext else None,
                              h["w"][:, s], d)
    g = g_ext if ext else g_pl
    fv.check_parity(fv.contract([a[:, s] for a in g[1:]], d), ref, err, f"{case} gpu ext={ext}")


@pytest.mark.parametrize("case", MODELS)
def test_qdd_is_fd_ext(ffi, case):
    mb, _, _, _, dev, t_ext, _, _, _ = _case(case)
    assert torch.equal(t_ext[0], mb.fd_ext_batch(dev["q"], dev["qd"], dev["tau"], dev["fext"]))


@pytest.mark.parametrize("case", MODELS)
def test_identities(ffi, case):
    """sym(H) g_tau = w (crba_batch) and g_fext = link_vel_batch(q, g_tau) on all 257 configurations."""
    mb, _, _, h, dev, t_ext, t_pl, g_ext, g_pl = _case(case)
    n = mb.n
    H = mb.crba_batch(dev["q"]).cpu().numpy().reshape(n, n, B)  # element row + n col: [col, row, b]
    Hs = np.zeros((n, n, B))
    for i in range(n):
        for k in range(n):
            Hs[i, k] = H[max(i, k), min(i, k)]  # the upper triangle (row <= col) is the ABI's
    e0 = max(fv.scaled(np.einsum("ikb,kb->ib", Hs, g[3]), h["w"]) for g in (g_ext, g_pl))
    e1 = fv.scaled(g_ext[4], mb.link_vel_batch(dev["q"], t_ext[3]).cpu().numpy())
    print(f"{case} fd_vjp gpu identities: sym(H) g_tau {e0:.3e} link_vel {e1:.3e}")
    assert e0 <= 1e-9 and e1 <= 1e-9


@pytest.mark.parametrize("case", MODELS)
def test_plain_equals_zero_wrench(ffi, case):
    """Bit for bit."""
    mb, _, _, _, dev, _, t_pl, _, _ = _case(case)
    g0 = mb.fd_vjp_batch(dev["q"], dev["qd"], dev["tau"], dev["w"], fext=_rows(np.zeros((6 * mb.n, B))))
    for k in range(4):
        assert torch.equal(g0[k], t_pl[k]), (case, k, (g0[k] - t_pl[k]).abs().max().item())


@pytest.mark.parametrize("case", MODELS)
def test_against_the_composition(ffi, case):
    """g_q, g_qd, g_fext against -rnea_vjp_batch(q, qd, qdd, g_tau, fext), the documented composition's last
    step, at this kernel's own qdd and g_tau: g_qd and g_fext bit for bit, g_q to COMPOSITION_BOUND."""
    mb, _, _, _, dev, t_ext, _, _, _ = _case(case)
    c = mb.rnea_vjp_batch(dev["q"], dev["qd"], t_ext[0], t_ext[3], fext=dev["fext"])
    diff = [fv.scaled(-c[a].cpu().numpy(), t_ext[b].cpu().numpy()) for a, b in ((0, 1), (1, 2), (3, 4))]
    print(f"{case} fd_vjp against the composition: q {diff[0]:.3e} qd {diff[1]:.3e} fext {diff[2]:.3e}")
    assert torch.equal(-c[1], t_ext[2]) and torch.equal(-c[3], t_ext[4])
    assert diff[0] <= COMPOSITION_BOUND


@pytest.mark.parametrize("case", ["fr3", "chain16"])
def test_kernel_against_host_form(ffi, case):
    mb, _, _, h, _, _, _, g_ext, _ = _case(case)
    worst = 0.0
    for b in range(0, B, 8):
        g = mb.fd_vjp(h["q"][:, b], h["qd"][:, b], h["tau"][:, b], h["w"][:, b], h["fext"][:, b])
        worst = max(worst, *[fv.scaled(g_ext[k][:, b], np.asarray(g[k]).reshape(-1)) for k in range(5)])
    print(f"{case} fd_vjp kernel against host form: {worst:.3e}")
    assert worst <= HOST_FORM_BOUND


@pytest.mark.parametrize("case", ["fr3", "tree9", "floating14"])
def test_f32_against_f64(ffi, case):
    """fp32 against the fp64 kernel on the same fp32-rounded inputs, per configuration and output array."""
    mb, _, _, h, _, _, _, _, _ = _case(case)
    t32 = {k: _rows(v, torch.float32, 0) for k, v in h.items()}
    t64 = {k: v.double() for k, v in t32.items()}
    g32 = mb.fd_vjp_batch(t32["q"], t32["qd"], t32["tau"], t32["w"], fext=t32["fext"])
    g64 = mb.fd_vjp_batch(t64["q"], t64["qd"], t64["tau"], t64["w"], fext=t64["fext"])
    worst = 0.0
    for a, r in zip(g32, g64):
        assert a.dtype == torch.float32
        a, r = a.double().cpu().numpy(), r.cpu().numpy()
        worst = max(worst, (np.abs(a - r).max(axis=0) / (1.0 + np.abs(r).max(axis=0))).max())
    print(f"{case} fd_vjp fp32 against fp64: {worst:.3e}")
    assert worst <= F32_BOUND


@pytest.mark.parametrize("case", ["fr3", "tree9"])
def test_input_domain(ffi, case):
    mb, _, _, _, dev, _, _, g_ext, _ = _case(case)
    others = [b for b in range(B) if b != 17]
    pri = re.search(r"kPri\[N\] = \{([^}]*)\}", mb.fd_vjp_jit_source(True, True))
    rev = 1 if pri is None else [int(t) for t in pri.group(1).split(",")].index(0)  # a revolute joint's row
    # a NaN position, an Inf wrench row, an angle past the fp64 bound (2^41), a NaN torque
    for name, row, bad in (("q", 1, float("nan")), ("fext", 1, float("inf")), ("q", rev, 1.0e13), ("tau", 1, float("nan"))):
        x = {k: v.clone() for k, v in dev.items()}
        x[name][row, 17] = bad
        g = [t.cpu().numpy() for t in mb.fd_vjp_batch(x["q"], x["qd"], x["tau"], x["w"], fext=x["fext"])]
        for k in range(5):
            assert np.isnan(g[k][:, 17]).all(), (case, name, bad, k)
            assert np.array_equal(g[k][:, others], g_ext[k][:, others]), (case, name, bad, k)
    x = {k: v.clone() for k, v in dev.items()}
    x["w"][1, 17] = float("nan")  # not checked: propagates by arithmetic, in its own configuration only
    g = [t.cpu().numpy() for t in mb.fd_vjp_batch(x["q"], x["qd"], x["tau"], x["w"], fext=x["fext"])]
    for k in range(5):
        assert np.array_equal(g[k][:, others], g_ext[k][:, others]), (case, k)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_pointer_forms_equal_device_forms(ffi, dtype):
    mb, _, _, h, _, _, _, _, _ = _case("fr3")
    a = {k: np.ascontiguousarray(v, dtype=dtype) for k, v in h.items()}
    t = {k: torch.as_tensor(v, device=DEV) for k, v in a.items()}
    for fext in (True, False):
        gh = mb.fd_vjp_batch_host(a["q"], a["qd"], a["tau"], a["w"], fext=a["fext"] if fext else None, dtype=dtype)
        gd = mb.fd_vjp_batch(t["q"], t["qd"], t["tau"], t["w"], fext=t["fext"] if fext else None)
        assert len(gh) == len(gd) == (5 if fext else 4)
        for x, y in zip(gh, gd):
            assert x.dtype == dtype and np.array_equal(x, y.cpu().numpy())


def test_without_hiprtc(ffi):
    """Both families, fp32 and fp64, at the C entry points: RB_ERR_UNSUPPORTED (6) with the reason."""
    mb, _, _ = fv.setup("fr3")
    lib = ffi.lib()
    ffi.set_tuning("jit", 0)
    try:
        for t, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            for kind, k, wide in (("fd_vjp", 10, (3, 9)), ("fd_vjp_plain", 8, ())):
                bufs = [torch.zeros(((6 if i in wide else 1) * mb.n, 4), dtype=dtype, device=DEV) for i in range(k)]
                rc = getattr(lib, f"multibody_{kind}_batch_{t}")(mb.handle, *[b.data_ptr() for b in bufs], 4, 4, None)
                assert rc == 6 and "hipRTC" in ffi.last_error(), (kind, t, rc, ffi.last_error())
        z = torch.zeros((mb.n, 4), dtype=torch.float64, device=DEV)
        with pytest.raises(ffi.RigidBodyError, match="hipRTC"):
            mb.fd_vjp_batch(z, z, z, z)
    finally:
        ffi.set_tuning("jit", 1)


@pytest.mark.parametrize("case,ext", [("fr3", False), ("floating14", True)])
def test_autograd_gradcheck(ffi, case, ext):
    from rigidbody_amd import autograd

    mb, _, _, h, _, _, _, _, _ = _case(case)
    names = ("q", "qd", "tau") + (("fext",) if ext else ())
    ins = [torch.as_tensor(np.ascontiguousarray(h[k][:, :3]), device=DEV).requires_grad_(True) for k in names]
    assert torch.autograd.gradcheck(lambda *a: autograd.fd(mb, *a), ins, eps=1e-6, atol=1e-5, rtol=1e-4)


def test_autograd_backward_f32(ffi):
    from rigidbody_amd import autograd

    mb, _, _, h, _, _, _, _, _ = _case("fr3")
    q, qd, tau, fext = (torch.as_tensor(np.ascontiguousarray(h[k][:, :5], dtype=np.float32), device=DEV)
                        for k in ("q", "qd", "tau", "fext"))
    q.requires_grad_(True)
    fext.requires_grad_(True)
    before = [t.detach().clone() for t in (q, qd, tau, fext)]
    qdd = autograd.fd(mb, q, qd, tau, fext)
    assert qdd.shape == (mb.n, 5) and qdd.dtype == torch.float32
    qdd.square().sum().backward()
    assert q.grad.shape == q.shape and q.grad.dtype == torch.float32 and fext.grad.shape == fext.shape
    assert qd.grad is None and tau.grad is None
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, (q, qd, tau, fext)))
