"""The reverse-mode gradient of the inverse dynamics on the GPU (multibody_rnea_vjp_batch_* /
multibody_rnea_vjp_plain_batch_*, rnea_vjp_body.hip.hpp) and its torch.autograd wrapper.  B = 257: one
full 256-lane block plus a one-lane tail; fp64 runs on rows of leading dimension B + 3.  Reference:
tests/rnea_vjp_ref.py; bounds are the header's contracts."""
import numpy as np
import pytest
import torch

import rnea_vjp_ref as rv

pytestmark = pytest.mark.gpu

B, NREF = 257, 40
MODELS = ["fr3", "general12", "chain16", "tree9", "floating14"]
DEV = "cuda:0"
_CACHE = {}


@pytest.fixture(scope="module")
def ffi():
    from rigidbody_amd import ffi

    if not hasattr(ffi.Multibody, "rnea_vjp_batch"):
        pytest.fail("the binding has no rnea_vjp entry points")
    return ffi


def _rows(x, dtype=torch.float64, pad=3):
    """[rows, B] on the device, on rows of leading dimension B + pad."""
    t = torch.empty((x.shape[0], x.shape[1] + pad), dtype=dtype, device=DEV)[:, :x.shape[1]]
    t.copy_(torch.as_tensor(x))
    return t


def _case(case):
    """Model, host inputs, device inputs and both kernels' fp64 outputs (numpy), computed once."""
    if case not in _CACHE:
        mb, om, m6 = rv.setup(case)
        q, qd, qdd, _, fext = rv.inputs(mb, B, 91)
        w = rv.cotangent(mb, B, 92)
        host = dict(q=q, qd=qd, qdd=qdd, fext=fext, w=w)
        dev = {k: _rows(v) for k, v in host.items()}
        g_ext = mb.rnea_vjp_batch(dev["q"], dev["qd"], dev["qdd"], dev["w"], fext=dev["fext"])
        g_pl = mb.rnea_vjp_batch(dev["q"], dev["qd"], dev["qdd"], dev["w"])
        assert len(g_ext) == 4 and len(g_pl) == 3
        _CACHE[case] = (mb, om, m6, host, dev, [t.cpu().numpy() for t in g_ext], [t.cpu().numpy() for t in g_pl])
    return _CACHE[case]


@pytest.mark.parametrize("case,ext", [(c, True) for c in MODELS] + [("fr3", False), ("floating14", False)])
def test_reference_parity_f64(ffi, case, ext):
    mb, om, m6, h, _, g_ext, g_pl = _case(case)
    d = rv.direction(mb, NREF, 93, ext)
    s = slice(0, NREF)
    ref, err = rv.directional(om, m6, h["q"][:, s], h["qd"][:, s], h["qdd"][:, s], h["fext"][:, s] if ext else None,
                              h["w"][:, s], d)
    g = g_ext if ext else g_pl
    rv.check_parity(rv.contract([a[:, s] for a in g], d), ref, err, f"{case} gpu ext={ext}")


@pytest.mark.parametrize("case", MODELS)
def test_identities(ffi, case):
    """g_qdd = sym(H) w (crba_batch) and g_fext = -link_vel_batch(q, w) on all 257 configurations."""
    mb, _, _, h, dev, g_ext, g_pl = _case(case)
    n = mb.n
    H = mb.crba_batch(dev["q"]).cpu().numpy().reshape(n, n, B)  # element row + n col: [col, row, b]
    Hs = np.zeros((n, n, B))
    for i in range(n):
        for k in range(n):
            Hs[i, k] = H[max(i, k), min(i, k)]  # the upper triangle (row <= col) is the ABI's
    hw = np.einsum("ikb,kb->ib", Hs, h["w"])
    e0 = max(rv.scaled(g_ext[2], hw), rv.scaled(g_pl[2], hw))
    e1 = rv.scaled(g_ext[3], -mb.link_vel_batch(dev["q"], dev["w"]).cpu().numpy())
    print(f"{case} rnea_vjp gpu identities: sym(H) w {e0:.3e} link_vel {e1:.3e}")
    assert e0 <= 1e-9 and e1 <= 1e-9


@pytest.mark.parametrize("case", ["fr3", "general12", "chain16"])
def test_against_rnea_deriv(ffi, case):
    mb, _, _, h, dev, _, g_pl = _case(case)
    n = mb.n
    dq, dqd = (t.cpu().numpy().reshape(n, n, B) for t in mb.rnea_deriv_batch(dev["q"], dev["qd"], dev["qdd"]))
    e = [rv.scaled(g_pl[k], np.einsum("kib,ib->kb", m, h["w"])) for k, m in enumerate((dq, dqd))]  # [k, i]: row i + n k
    print(f"{case} rnea_vjp against rnea_deriv: q {e[0]:.3e} qd {e[1]:.3e}")
    assert max(e) <= 1e-8


@pytest.mark.parametrize("case", MODELS)
def test_plain_equals_zero_wrench(ffi, case):
    mb, _, _, _, dev, _, g_pl = _case(case)
    g0 = mb.rnea_vjp_batch(dev["q"], dev["qd"], dev["qdd"], dev["w"], fext=_rows(np.zeros((6 * mb.n, B))))
    e = max(rv.scaled(g0[k].cpu().numpy(), g_pl[k]) for k in range(3))
    print(f"{case} rnea_vjp plain against zero wrench: {e:.3e}")
    assert e <= 1e-12


@pytest.mark.parametrize("case", ["fr3", "chain16"])
def test_kernel_against_host_form(ffi, case):
    """Measured on the MI355X: 2.52e-15 at most (16 links; FR3 1.33e-15); the bound is 10x that."""
    mb, _, _, h, _, g_ext, _ = _case(case)
    worst = 0.0
    for b in range(0, B, 8):
        g = mb.rnea_vjp(h["q"][:, b], h["qd"][:, b], h["qdd"][:, b], h["w"][:, b], h["fext"][:, b])
        worst = max(worst, *[rv.scaled(g_ext[k][:, b], np.asarray(g[k]).reshape(-1)) for k in range(4)])
    print(f"{case} rnea_vjp kernel against host form: {worst:.3e}")
    assert worst <= 2.52e-14


@pytest.mark.parametrize("case", ["fr3", "tree9", "floating14"])
def test_f32_against_f64(ffi, case):
    """fp32 against the fp64 kernel on the same fp32-rounded inputs, per configuration and output array.
    Measured on the MI355X: 2.71e-6 at most (floating base; FR3 8.4e-7, the 9-joint tree 7.8e-7); the bound is
    7x that, rounded."""
    mb, _, _, h, _, _, _ = _case(case)
    t32 = {k: _rows(v, torch.float32, 0) for k, v in h.items()}
    t64 = {k: v.double() for k, v in t32.items()}
    g32 = mb.rnea_vjp_batch(t32["q"], t32["qd"], t32["qdd"], t32["w"], fext=t32["fext"])
    g64 = mb.rnea_vjp_batch(t64["q"], t64["qd"], t64["qdd"], t64["w"], fext=t64["fext"])
    worst = 0.0
    for a, r in zip(g32, g64):
        assert a.dtype == torch.float32
        a, r = a.double().cpu().numpy(), r.cpu().numpy()
        worst = max(worst, (np.abs(a - r).max(axis=0) / (1.0 + np.abs(r).max(axis=0))).max())
    print(f"{case} rnea_vjp fp32 against fp64: {worst:.3e}")
    assert worst <= 2e-5


@pytest.mark.parametrize("case", ["fr3", "tree9"])
def test_input_domain(ffi, case):
    mb, _, _, _, dev, g_ext, _ = _case(case)
    others = [b for b in range(B) if b != 17]
    for name, bad in (("q", float("nan")), ("fext", float("inf")), ("qdd", float("nan"))):
        x = {k: v.clone() for k, v in dev.items()}
        x[name][1, 17] = bad
        g = [t.cpu().numpy() for t in mb.rnea_vjp_batch(x["q"], x["qd"], x["qdd"], x["w"], fext=x["fext"])]
        for k in range(4):
            assert np.isnan(g[k][:, 17]).all(), (case, name, k)
            assert np.array_equal(g[k][:, others], g_ext[k][:, others]), (case, name, k)
    x = {k: v.clone() for k, v in dev.items()}
    x["w"][1, 17] = float("nan")  # not checked: propagates by arithmetic, in its own configuration only
    g = [t.cpu().numpy() for t in mb.rnea_vjp_batch(x["q"], x["qd"], x["qdd"], x["w"], fext=x["fext"])]
    for k in range(4):
        assert np.array_equal(g[k][:, others], g_ext[k][:, others]), (case, k)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_pointer_forms_equal_device_forms(ffi, dtype):
    mb, _, _, h, _, _, _ = _case("fr3")
    a = {k: np.ascontiguousarray(v, dtype=dtype) for k, v in h.items()}
    t = {k: torch.as_tensor(v, device=DEV) for k, v in a.items()}
    for fext in (True, False):
        gh = mb.rnea_vjp_batch_host(a["q"], a["qd"], a["qdd"], a["w"], fext=a["fext"] if fext else None, dtype=dtype)
        gd = mb.rnea_vjp_batch(t["q"], t["qd"], t["qdd"], t["w"], fext=t["fext"] if fext else None)
        assert len(gh) == len(gd) == (4 if fext else 3)
        for x, y in zip(gh, gd):
            assert x.dtype == dtype and np.array_equal(x, y.cpu().numpy())


def test_without_hiprtc(ffi):
    mb, _, _ = rv.setup("fr3")
    z = torch.zeros((mb.n, 4), dtype=torch.float64, device=DEV)
    ffi.set_tuning("jit", 0)
    try:
        with pytest.raises(ffi.RigidBodyError, match="hipRTC"):
            mb.rnea_vjp_batch(z, z, z, z)
    finally:
        ffi.set_tuning("jit", 1)


@pytest.mark.parametrize("case,ext", [("fr3", False), ("floating14", True)])
def test_autograd_gradcheck(ffi, case, ext):
    from rigidbody_amd import autograd

    mb, _, _, h, _, _, _ = _case(case)
    names = ("q", "qd", "qdd") + (("fext",) if ext else ())
    ins = [torch.as_tensor(np.ascontiguousarray(h[k][:, :2]), device=DEV).requires_grad_(True) for k in names]
    assert torch.autograd.gradcheck(lambda *a: autograd.rnea(mb, *a), ins, eps=1e-6, atol=1e-5, rtol=1e-4)


def test_autograd_backward_f32(ffi):
    from rigidbody_amd import autograd

    mb, _, _, h, _, _, _ = _case("fr3")
    q, qd, qdd, fext = (torch.as_tensor(np.ascontiguousarray(h[k][:, :5], dtype=np.float32), device=DEV)
                        for k in ("q", "qd", "qdd", "fext"))
    q.requires_grad_(True)
    fext.requires_grad_(True)
    before = [t.detach().clone() for t in (q, qd, qdd, fext)]
    tau = autograd.rnea(mb, q, qd, qdd, fext)
    assert tau.shape == (mb.n, 5) and tau.dtype == torch.float32
    tau.square().sum().backward()
    assert q.grad.shape == q.shape and q.grad.dtype == torch.float32 and fext.grad.shape == fext.shape
    assert qd.grad is None and qdd.grad is None
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, (q, qd, qdd, fext)))
