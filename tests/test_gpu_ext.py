"""External link wrenches on the GPU: multibody_rnea_ext_batch_* / multibody_fd_ext_batch_* against
tests/ext_wrench_ref.py (the fp64 oracle plus J^T f composed from the 6x6 model's transforms).
Every batch is B = 257 -- one full 256-lane block and a one-lane tail -- and the fp64 parity runs
on rows of leading dimension B + 3.  Bounds: the header's (fp64 1e-9 / residual 1e-8 / 1e-7 as
tests/test_gpu_tree.py holds the plain forward dynamics to; fp32 1e-4 and 1e-3 norm-wise)."""
import numpy as np
import pytest

import ext_wrench_ref as xr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B = 257
MODELS = ["fr3", "general12", "chain16", "tree9", "floating14"]  # mass-matrix FD: the first two
_cache = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _case(case):
    """Model, inputs and reference of one case, computed once and never modified."""
    if case not in _cache:
        mb, om, m6 = xr.setup(case)
        q, qd, qdd, tau, fext = xr.inputs(mb, B, 41)
        jtf = xr.jt_f_batch(m6, q, fext)
        _cache[case] = dict(mb=mb, om=om, x=(q, qd, qdd, tau, fext), jtf=jtf,
                            tau_ref=om.rnea_batch(q, qd, qdd) - jtf, qdd_ref=om.fd_batch(q, qd, tau + jtf))
        for a in (q, qd, qdd, tau, fext, jtf, _cache[case]["tau_ref"], _cache[case]["qdd_ref"]):
            a.setflags(write=False)
    return _cache[case]


def _t(a, dev, dtype=torch.float64, pad=0):
    """[rows, B] device tensor; pad > 0: a view of rows of leading dimension B + pad."""
    a = np.array(a)  # a writable copy: the cached inputs are read-only
    t = torch.zeros((a.shape[0], a.shape[1] + pad), dtype=dtype, device=dev)
    t[:, : a.shape[1]] = torch.as_tensor(a, dtype=dtype, device=dev)
    return t[:, : a.shape[1]]


def _scaled(got, ref):
    got = np.asarray(got, float)
    assert np.all(np.isfinite(got)), "non-finite output"
    return (np.abs(got - ref) / (1.0 + np.abs(ref))).max()


@pytest.mark.parametrize("case", MODELS)
def test_parity_f64(case, dev):
    c = _case(case)
    mb, om = c["mb"], c["om"]
    q, qd, qdd, tau, fext = c["x"]
    tq, tqd, tqdd, ttau, tf = (_t(a, dev, pad=3) for a in (q, qd, qdd, tau, fext))
    assert tq.stride(0) == B + 3
    got = mb.rnea_ext_batch(tq, tqd, tqdd, tf)
    assert got.stride(0) == B + 3
    err = _scaled(got.cpu().numpy(), c["tau_ref"])
    print(f"{case} rnea_ext f64 {err:.3e}")
    assert err <= 1e-9
    acc = mb.fd_ext_batch(tq, tqd, ttau, tf).cpu().numpy()
    drive = tau + c["jtf"]
    res = (np.abs(om.rnea_batch(q, qd, acc) - drive) / (1 + np.abs(drive))).max()
    err = _scaled(acc, c["qdd_ref"])
    print(f"{case} fd_ext f64 residual {res:.3e} qdd {err:.3e}")
    assert res <= 1e-8
    assert err <= 1e-7


@pytest.mark.parametrize("case", MODELS)
def test_zero_wrench_is_the_plain_dynamics(case, dev):
    c = _case(case)
    mb = c["mb"]
    q, qd, qdd, tau, fext = (_t(a, dev) for a in c["x"])
    zero = torch.zeros_like(fext)
    e1 = _scaled(mb.rnea_ext_batch(q, qd, qdd, zero).cpu().numpy(), mb.rnea_batch(q, qd, qdd).cpu().numpy())
    e2 = _scaled(mb.fd_ext_batch(q, qd, tau, zero).cpu().numpy(), mb.fd_batch(q, qd, tau).cpu().numpy())
    print(f"{case} zero wrench rnea {e1:.3e} fd {e2:.3e}")
    assert e1 <= 1e-12 and e2 <= 1e-12


@pytest.mark.parametrize("case", ["fr3", "tree9"])
def test_last_link_wrench_is_jacobian_transpose(case, dev):
    c = _case(case)
    mb, n = c["mb"], c["mb"].n
    q, qd, qdd, _, fext = c["x"]
    last = np.zeros_like(fext)
    last[6 * (n - 1):] = fext[6 * (n - 1):]
    tq, tqd, tqdd = (_t(a, dev) for a in (q, qd, qdd))
    d = (mb.rnea_batch(tq, tqd, tqdd) - mb.rnea_ext_batch(tq, tqd, tqdd, _t(last, dev))).cpu().numpy()
    J = mb.jac_batch(tq).cpu().numpy().reshape(n, 6, B)  # [column, row (lin; rot), b]
    ref = np.einsum("jcb,cb->jb", J, last[6 * (n - 1):])
    assert _scaled(d, ref) <= 1e-9


@pytest.mark.parametrize("case", ["fr3", "tree9", "floating14"])
def test_f32_against_f64_kernel(case, dev):
    c = _case(case)
    mb = c["mb"]
    f = torch.float32
    x32 = [a.astype(np.float32).astype(np.float64) for a in c["x"]]
    q, qd, qdd, tau, fext = x32
    t32 = [_t(a, dev, f) for a in x32]
    t64 = [_t(a, dev) for a in x32]
    got = mb.rnea_ext_batch(t32[0], t32[1], t32[2], t32[4]).cpu().numpy().astype(np.float64)
    ref = mb.rnea_ext_batch(t64[0], t64[1], t64[2], t64[4]).cpu().numpy()
    assert np.all(np.isfinite(got))
    e = np.abs(got - ref).max(axis=0) / (1 + np.abs(ref).max(axis=0))
    print(f"{case} rnea_ext f32 norm-wise {e.max():.3e} at configuration {e.argmax()}")
    assert e.max() <= 1e-4
    acc = mb.fd_ext_batch(t32[0], t32[1], t32[3], t32[4]).cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(acc))
    # the torque residual through the fp64 kernel: rnea_ext(q, qd, acc, fext) against tau
    back = mb.rnea_ext_batch(t64[0], t64[1], _t(acc, dev), t64[4]).cpu().numpy()
    r = np.abs(back - tau).max(axis=0) / (1 + np.abs(tau + c["jtf"]).max(axis=0))  # scale: the driving torque
    print(f"{case} fd_ext f32 residual norm-wise {r.max():.3e} at configuration {r.argmax()}")
    assert r.max() <= 1e-3


@pytest.mark.parametrize("case", ["fr3", "tree9"])
def test_input_domain(case, dev):
    c = _case(case)
    mb = c["mb"]
    q, qd, qdd, tau, fext = (_t(a, dev) for a in c["x"])
    clean = (mb.rnea_ext_batch(q, qd, qdd, fext).cpu().numpy(), mb.fd_ext_batch(q, qd, tau, fext).cpu().numpy())
    keep = np.ones(B, bool)
    keep[17] = False
    for which, row, bad in (("fext", 4, float("nan")), ("fext", 6 * mb.n - 1, float("inf")), ("q", 1, float("nan"))):
        qb, fb = q.clone(), fext.clone()
        (fb if which == "fext" else qb)[row, 17] = bad
        outs = (mb.rnea_ext_batch(qb, qd, qdd, fb).cpu().numpy(), mb.fd_ext_batch(qb, qd, tau, fb).cpu().numpy())
        for got, ref in zip(outs, clean):
            assert np.isnan(got[:, 17]).all(), (which, row, bad)
            assert np.array_equal(got[:, keep], ref[:, keep]), (which, row, bad)


def test_host_pointer_forms_equal_device_forms(dev):
    c = _case("fr3")
    mb = c["mb"]
    q, qd, qdd, tau, fext = c["x"]
    t = [_t(a, dev) for a in c["x"]]
    assert np.array_equal(mb.rnea_ext_batch_host(q, qd, qdd, fext), mb.rnea_ext_batch(t[0], t[1], t[2], t[4]).cpu().numpy())
    assert np.array_equal(mb.fd_ext_batch_host(q, qd, tau, fext), mb.fd_ext_batch(t[0], t[1], t[3], t[4]).cpu().numpy())
    f = np.float32
    t32 = [_t(a, dev, torch.float32) for a in c["x"]]
    assert np.array_equal(mb.rnea_ext_batch_host(q, qd, qdd, fext, dtype=f),
                          mb.rnea_ext_batch(t32[0], t32[1], t32[2], t32[4]).cpu().numpy())
    assert np.array_equal(mb.fd_ext_batch_host(q, qd, tau, fext, dtype=f),
                          mb.fd_ext_batch(t32[0], t32[1], t32[3], t32[4]).cpu().numpy())


def test_without_hiprtc_fails_loudly(dev):
    from rigidbody_amd import ffi

    mb = _case("fr3")["mb"]
    z = torch.zeros((mb.n, 8), dtype=torch.float64, device=dev)
    fz = torch.zeros((6 * mb.n, 8), dtype=torch.float64, device=dev)
    try:
        ffi.set_tuning("jit", 0)
        with pytest.raises(ffi.RigidBodyError, match="hipRTC"):
            mb.rnea_ext_batch(z, z, z, fz)
        with pytest.raises(ffi.RigidBodyError, match="hipRTC"):
            mb.fd_ext_batch(z, z, z, fz)
    finally:
        ffi.set_tuning("jit", 1)
