"""multibody_rnea_deriv_batch_* / multibody_fd_deriv_batch_* on the GPU (hipRTC kinds 7 / 8,
rnea_deriv_body.hip.hpp) against the reference of deriv_ref.py: Richardson-extrapolated central
differences of the fp64 oracle on the same (for fp32: fp32-rounded) inputs, its own consistency
asserted first (1e-9 scaled; measured 6e-11 on these inputs).

fp64: 1e-8 (1 + |ref|) element-wise; the forward-dynamics matrices through their defining
identities with sym(H) from the oracle (1e-9 / 1e-8 scaled), qdd bit-identical to fd_batch.
fp32, FR3 over its limits, measured on an MI355X: rnea derivatives, per column
max_i |d_ik| / (1 + max_i |ref_ik|), 2.2e-6 over 1000 configurations -- below 2.5e-5, so the bound
is the project's fp32 RNEA contract, 1e-4; forward-dynamics derivatives as row-sum residuals
|H_s X + dtau_ref| <= c eps32 (|H_s| |X| + |dtau_ref|), measured c = 14.8 (the three matrices, 1000
configurations), bound 60 = 4x that rounded up; the fp32 forward-dynamics contract's own constant
is 24, above the measured value: the derivative columns solve as accurately as qdd itself.
"""
import ctypes

import numpy as np
import pytest

import deriv_ref
from test_gpu_parity import _oracle, _t

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EPS32 = 2.0 ** -24
BMAX = 1000
# fp32 bounds: the project's fp32 RNEA contract (measured value <= 2.5e-5, see above), and 4x the
# measured constant of the forward-dynamics residual, rounded up
RNEA32_TOL = 1e-4
FD32_C = 60.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ffi():
    from rigidbody_amd import ffi

    return ffi


_cache = {}


def _case(ffi, name, dt):
    """Model, oracle, inputs (q, qd, qdd, tau) [n, BMAX] in fp64 holding the values the kernel
    sees (fp32-rounded for dt = "f32"), and lazily the references -- computed once per module."""
    key = (name, dt)
    if key not in _cache:
        from rigidbody_amd import chains

        xml = chains.fr3_urdf_text() if name == "fr3" else chains.synthetic_chain_urdf(12)
        mb = ffi.Multibody.from_urdf_string(xml)
        B = BMAX if name == "fr3" else 300
        x = [chains.host_uniform(mb.n, B, *chains.input_ranges(mb.limits(), k), 900 + i)
             for i, k in enumerate(("q", "qd", "qdd", "tau"))]
        # tau: the torques of in-range accelerations.  Drawn over the effort limits they give
        # |qdd| ~ 1e3 on the distal joints, where differences of the oracle's rnea at that qdd are
        # self-consistent to 1.1e-9 only -- past the 1e-9 this reference must meet.
        om = _oracle(xml)
        x[3] = om.rnea_batch(x[0], x[1], x[2], nthreads=16)
        if dt == "f32":
            x = [a.astype(np.float32).astype(np.float64) for a in x]
        _cache[key] = {"mb": mb, "om": om, "x": x}
    return _cache[key]


def _rnea_ref(c):
    if "rnea_ref" not in c:
        q, qd, qdd, _ = c["x"]
        rq, rqd, cons = deriv_ref.rnea_deriv_ref(c["om"], q, qd, qdd)
        print(f"reference consistency {cons.max():.2e}")
        assert cons.max() <= 1e-9
        c["rnea_ref"] = (rq, rqd)
    return c["rnea_ref"]


def _fd_ref(c):
    """sym(H) [B, n, n], qdd = fd(q, qd, tau) and the rnea derivatives there, all from the oracle."""
    if "fd_ref" not in c:
        q, qd, _, tau = c["x"]
        om = c["om"]
        qdd = om.fd_batch(q, qd, tau, nthreads=16)
        rq, rqd, cons = deriv_ref.rnea_deriv_ref(om, q, qd, qdd)
        print(f"reference consistency {cons.max():.2e}")
        assert cons.max() <= 1e-9
        c["fd_ref"] = (deriv_ref.sym_h(om, q), qdd, deriv_ref.mats(rq), deriv_ref.mats(rqd))
    return c["fd_ref"]


def _dev_inputs(c, dev, dt, B, which=(0, 1, 2)):
    tdt = torch.float64 if dt == "f64" else torch.float32
    return [_t(c["x"][i][:, :B], dev, tdt) for i in which]


def _col_err(got, ref):
    """Per column k: max_i |d_ik| / (1 + max_i |ref_ik|), the largest over columns and configurations."""
    g, r = deriv_ref.mats(got), deriv_ref.mats(ref)
    assert np.all(np.isfinite(g)), "non-finite output"
    return float((np.abs(g - r).max(axis=1) / (1 + np.abs(r).max(axis=1))).max())


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("B", [1, 255, 257, 1000])
def test_rnea_deriv_fr3(ffi, dev, dt, B):
    c = _case(ffi, "fr3", dt)
    mb = c["mb"]
    assert mb.kernel_path("rnea_deriv", dt == "f64", B) == "jit"
    rq, rqd = _rnea_ref(c)
    dq, dqd = mb.rnea_deriv_batch(*_dev_inputs(c, dev, dt, B))
    assert dq.shape == (49, B) and dqd.shape == (49, B)
    dq, dqd = dq.cpu().numpy(), dqd.cpu().numpy()
    if dt == "f64":
        err = max(deriv_ref.scaled(dq, rq[:, :B]), deriv_ref.scaled(dqd, rqd[:, :B]))
        print(f"rnea_deriv f64 B={B}: max scaled error {err:.2e}")
        assert err <= 1e-8
    else:
        err = max(_col_err(dq, rq[:, :B]), _col_err(dqd, rqd[:, :B]))
        print(f"rnea_deriv f32 B={B}: max column error {err:.2e}")
        assert err <= RNEA32_TOL


def test_rnea_deriv_chain12(ffi, dev):
    c = _case(ffi, "chain12", "f64")
    mb, B = c["mb"], 300
    assert mb.kernel_path("rnea_deriv", True, B) == "jit"
    rq, rqd = _rnea_ref(c)
    dq, dqd = mb.rnea_deriv_batch(*_dev_inputs(c, dev, "f64", B))
    err = max(deriv_ref.scaled(dq.cpu().numpy(), rq), deriv_ref.scaled(dqd.cpu().numpy(), rqd))
    print(f"rnea_deriv chain12 f64: max scaled error {err:.2e}")
    assert err <= 1e-8


def test_host_body_equals_device_body(ffi, dev):
    """The same lane body compiled twice (host: origin-form link forces, libm-free sincos; device:
    centre-of-mass form, table sincos, FMA contraction): 1e-12 relative."""
    c = _case(ffi, "fr3", "f64")
    mb, B = c["mb"], 64
    q, qd, qdd = (c["x"][i][:, :B] for i in range(3))
    dq, dqd = (t.cpu().numpy() for t in mb.rnea_deriv_batch(*_dev_inputs(c, dev, "f64", B)))
    for b in range(B):
        hq, hqd = mb.rnea_deriv(q[:, b], qd[:, b], qdd[:, b])
        for got, ref in ((dq[:, b].reshape(7, 7).T, hq), (dqd[:, b].reshape(7, 7).T, hqd)):
            assert np.abs(got - ref).max() <= 1e-12 * (1 + np.abs(ref).max())


def test_want_subsets_and_ld(ffi, dev):
    """Only "q" / only "qd": bit-identical to both, the other array never written (through the C
    call, a sentinel-filled buffer passed nowhere stays, and a NULL is accepted); ld = B + 37: the
    columns past B keep their sentinel."""
    c = _case(ffi, "fr3", "f64")
    mb, B = c["mb"], 257
    x = _dev_inputs(c, dev, "f64", B)
    dq, dqd = mb.rnea_deriv_batch(*x)
    (oq,) = mb.rnea_deriv_batch(*x, want=("q",))
    (oqd,) = mb.rnea_deriv_batch(*x, want=("qd",))
    assert torch.equal(oq, dq) and torch.equal(oqd, dqd)
    rqd, rq = mb.rnea_deriv_batch(*x, want=("qd", "q"))
    assert torch.equal(rq, dq) and torch.equal(rqd, dqd)
    ld = B + 37
    wide = [torch.full((7, ld), 0.25, dtype=torch.float64, device=dev) for _ in range(3)]
    for w, t in zip(wide, x):
        w[:, :B] = t
    out = [torch.full((49, ld), -77.0, dtype=torch.float64, device=dev) for _ in range(2)]
    fn = ffi.lib().multibody_rnea_deriv_batch_f64
    s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert fn(mb.handle, *[w.data_ptr() for w in wide], out[0].data_ptr(), None, B, ld, s) == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(out[0][:, :B], dq) and bool((out[0][:, B:] == -77.0).all())
    assert bool((out[1] == -77.0).all())  # not requested: never written
    assert fn(mb.handle, *[w.data_ptr() for w in wide], None, out[1].data_ptr(), B, ld, s) == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(out[1][:, :B], dqd) and bool((out[1][:, B:] == -77.0).all())


def test_host_forms_skip_null_outputs(ffi, dev):
    """The blocking host forms with one output NULL (the wrappers never pass one): the device
    scratch offsets of the later outputs then depend on which are present.  Each result equals the
    device-pointer form's with the same output NULL bit for bit -- the same kernel, the same launch
    -- and the skipped output's host buffer is never written.  B = 257: one full block and a tail."""
    c = _case(ffi, "fr3", "f64")
    mb, B, n = c["mb"], 257, 7
    lib = ffi.lib()
    s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for name, which, rows, skip in (("fd_deriv", (0, 1, 3), (n, n * n, n * n, n * n), 1),
                                    ("rnea_deriv", (0, 1, 2), (n * n, n * n), 1)):
        host_in = [np.ascontiguousarray(c["x"][i][:, :B]) for i in which]
        dev_in = _dev_inputs(c, dev, "f64", B, which)
        dev_out = [torch.full((r, B), -77.0, dtype=torch.float64, device=dev) for r in rows]
        ptrs = [None if k == skip else o.data_ptr() for k, o in enumerate(dev_out)]
        fn = getattr(lib, f"multibody_{name}_batch_f64")
        assert fn(mb.handle, *[t.data_ptr() for t in dev_in], *ptrs, B, B, s) == 0, ffi.last_error()
        torch.cuda.synchronize(dev)
        host_out = [np.full((r, B), -77.0) for r in rows]
        hptrs = [None if k == skip else o.ctypes.data for k, o in enumerate(host_out)]
        fn = getattr(lib, f"multibody_{name}_batch_host_f64")
        assert fn(mb.handle, *[a.ctypes.data for a in host_in], *hptrs, B) == 0, ffi.last_error()
        for k, (h, d) in enumerate(zip(host_out, dev_out)):
            if k == skip:
                assert np.all(h == -77.0) and bool((d == -77.0).all()), (name, k)  # untouched
            else:
                assert np.all(np.isfinite(h)), (name, k)
                assert np.array_equal(h.view(np.int64), d.cpu().numpy().view(np.int64)), (name, k)  # bit for bit


def _fd_identities(c, outs, B):
    """(|H X_tau - I|, |H X_q + dtau_dq|, |H X_qd + dtau_dqd|) scaled, fp64 outputs."""
    Hs, _, rq, rqd = _fd_ref(c)
    Hs, rq, rqd = Hs[:B], rq[:B], rqd[:B]
    fq, fqd, ft = (deriv_ref.mats(o.cpu().numpy()) for o in outs)
    n = Hs.shape[1]
    return (deriv_ref.scaled(Hs @ ft, np.broadcast_to(np.eye(n), ft.shape)), deriv_ref.scaled(Hs @ fq, -rq),
            deriv_ref.scaled(Hs @ fqd, -rqd))


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("B", [1, 257, 1000])
def test_fd_deriv_fr3(ffi, dev, dt, B):
    c = _case(ffi, "fr3", dt)
    mb = c["mb"]
    assert mb.kernel_path("fd_deriv", dt == "f64", B) == "jit"
    x = _dev_inputs(c, dev, dt, B, (0, 1, 3))
    qdd, fq, fqd, ft = mb.fd_deriv_batch(*x)
    assert torch.equal(qdd, mb.fd_batch(*x))
    if dt == "f64":
        inv, idq, idqd = _fd_identities(c, (fq, fqd, ft), B)
        print(f"fd_deriv f64 B={B}: H X_tau - I {inv:.2e}, H X_q + dtau_dq {idq:.2e}, H X_qd + dtau_dqd {idqd:.2e}")
        assert inv <= 1e-9 and idq <= 1e-8 and idqd <= 1e-8
        ftm = deriv_ref.mats(ft.cpu().numpy())  # full symmetric: both triangles written
        assert deriv_ref.scaled(ftm, ftm.transpose(0, 2, 1)) <= 1e-12
        return
    Hs, _, rq, rqd = _fd_ref(c)
    worst = 0.0
    for X, ref in ((fq, rq), (fqd, rqd), (ft, -np.broadcast_to(np.eye(7), rq.shape))):
        X = deriv_ref.mats(X.cpu().numpy())
        assert np.all(np.isfinite(X))
        res = np.abs(Hs[:B] @ X + ref[:B]).sum(axis=2)
        scale = (np.abs(Hs[:B]) @ np.abs(X) + np.abs(ref[:B])).sum(axis=2)
        worst = max(worst, float((res / (EPS32 * scale)).max()))
    print(f"fd_deriv f32 B={B}: residual constant c = {worst:.2f}")
    assert worst <= FD32_C


def test_fd_deriv_chain12(ffi, dev):
    c = _case(ffi, "chain12", "f64")
    mb, B = c["mb"], 300
    assert mb.kernel_path("fd_deriv", True, B) == "jit"
    x = _dev_inputs(c, dev, "f64", B, (0, 1, 3))
    qdd, fq, fqd, ft = mb.fd_deriv_batch(*x)
    assert torch.equal(qdd, mb.fd_batch(*x))
    inv, idq, idqd = _fd_identities(c, (fq, fqd, ft), B)
    print(f"fd_deriv chain12: H X_tau - I {inv:.2e}, H X_q + dtau_dq {idq:.2e}, H X_qd + dtau_dqd {idqd:.2e}")
    assert inv <= 1e-9 and idq <= 1e-8 and idqd <= 1e-8


def test_domain(ffi, dev):
    """NaN / Inf / an angle past the bound poison every output element of their configuration
    and nothing else."""
    c = _case(ffi, "fr3", "f64")
    mb, B = c["mb"], 300
    q, qd, qdd, tau = (_t(c["x"][i][:, :B], dev) for i in range(4))
    clean = mb.rnea_deriv_batch(q, qd, qdd) + mb.fd_deriv_batch(q, qd, tau)
    q, qd = q.clone(), qd.clone()
    q[3, 17] = float("nan")
    qd[0, 101] = float("inf")
    q[6, 200] = 2.0 ** 42
    bad = [17, 101, 200]
    good = torch.ones(B, dtype=torch.bool, device=dev)
    good[bad] = False
    for got, ref in zip(mb.rnea_deriv_batch(q, qd, qdd) + mb.fd_deriv_batch(q, qd, tau), clean):
        assert bool(torch.isnan(got[:, bad]).all())
        assert torch.equal(got[:, good], ref[:, good])


def test_unsupported_models(ffi, dev):
    from rigidbody_amd import chains

    tree = ffi.Multibody.from_urdf_string(chains.tree_urdf(), ffi.URDF_TREE | ffi.GENERAL_AXES)
    z = torch.zeros((tree.n, 8), dtype=torch.float64, device=dev)
    for call in (tree.rnea_deriv_batch, tree.fd_deriv_batch):
        with pytest.raises(ffi.RigidBodyError, match=r"status 6.*serial revolute"):
            call(z, z, z)
    c30 = ffi.Multibody.from_urdf_string(chains.synthetic_chain_urdf(30))
    z = torch.zeros((30, 8), dtype=torch.float32, device=dev)
    with pytest.raises(ffi.RigidBodyError, match=r"status 6.*mass-matrix"):
        c30.fd_deriv_batch(z, z, z)


def test_graph_capture(ffi, dev):
    """One rnea_deriv_batch (a single kernel) captured after upload() and replayed once."""
    c = _case(ffi, "fr3", "f64")
    mb, B = c["mb"], 1000
    x = _dev_inputs(c, dev, "f64", B)
    mb.upload()
    eager = mb.rnea_deriv_batch(*x)  # also compiles the kernel before the capture
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = mb.rnea_deriv_batch(*x)
    for o in out:
        o.zero_()
    g.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
