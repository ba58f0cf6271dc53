"""Compliant ground contact on the GPU: multibody_contact_wrench_batch_* and the fused
multibody_rollout_contact_batch_* against tests/contact_ref.py (the header's law on link_kin_ref, the
oracle's forward dynamics under the wrench) and against the composition of the existing entry points
(contact_wrench, fd_ext, the two fused multiply-add updates).  Every batch is B = 257 -- one full
256-lane block and a one-lane tail -- on rows of leading dimension 300.  Bounds: the header's (fp64
wrench 1e-9 scaled; trajectories 1e-7 scaled, the fd_ext contract -- a step scales its acceleration
error by dt = 1e-3, so that bound cannot be tight for the wrong reason; fp32 wrench 1e-4 norm-wise,
the rnea_ext contract).

The fp32 rollout (K = 4, against the fp64 kernel on fp32-rounded inputs, norm-wise per configuration
and array) had no contract: its bound, 4e-4, is 8x the maximum measured over the five models, 4.7e-5
(the 16-link chain's final qd), rounded up to one digit.

Measured on MI355X (this file's own prints): fp64 wrench against the reference 6.2e-13 at most
(general5 cforce); fused rollout against the composition 2.8e-14 at most (FR3 qd), against contact_ref
1.3e-13 (FR3 qd); fp32 wrench against the fp64 kernel 7.1e-5 at most (16 links), 1.7e-5 FR3; fp32
rollout traj 6.4e-6 at most (FR3), final qd 4.7e-5 at most (16 links)."""
import numpy as np
import pytest

import contact_ref as cr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, LD = 257, 300
SENTINEL = -7.25
MODELS = ["fr3", "chain16", "general5", "tree9", "floating14"]
_cache = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from rigidbody_amd import ffi

    if not hasattr(ffi.Multibody, "contact_wrench_batch"):
        pytest.fail("the binding has no contact entry points")
    return torch.device("cuda:0")


def _case(case):
    """Models, inputs and the wrench's reference of one case, computed once and never modified."""
    if case not in _cache:
        mb, plain, om, m6, cm, (q, qd, tau) = cr.setup(case, B, 81)
        rng = np.random.default_rng(82)
        tau_seq = np.stack([tau[:, rng.permutation(B)] for _ in range(4)])
        ref = cr.contact_batch(m6, cm, q, qd)
        _cache[case] = dict(mb=mb, plain=plain, om=om, m6=m6, cm=cm, x=(q, qd, tau_seq), ref=ref)
        for a in (q, qd, tau_seq, *ref):
            a.setflags(write=False)
    return _cache[case]


def _t(a, dev, dtype=torch.float64, fill=0.0):
    """[..., rows, B] view of a [..., rows, LD] device tensor whose padding columns hold `fill`."""
    a = np.array(a)  # a writable copy: the cached inputs are read-only
    t = torch.full((*a.shape[:-1], LD), fill, dtype=dtype, device=dev)
    t[..., :B] = torch.as_tensor(a, dtype=dtype, device=dev)
    return t[..., :B]


def _padded_out(shape, dev, dtype=torch.float64):
    full = torch.full((*shape, LD), SENTINEL, dtype=dtype, device=dev)
    return full, full[..., :B]


def _scaled(got, ref):
    got = np.asarray(got, float)
    assert np.all(np.isfinite(got)), "non-finite output"
    return (np.abs(got - ref) / (1.0 + np.abs(ref))).max()


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("case", MODELS)
def test_wrench_parity_f64(case, dev):
    c = _case(case)
    mb, n, P = c["mb"], c["mb"].n, len(c["cm"]["links"])
    share = cr.check_share(c["ref"][2])
    q, qd = (_t(a, dev) for a in c["x"][:2])
    assert q.stride(0) == LD
    (ff, fext), (fc, cforce) = _padded_out((6 * n,), dev), _padded_out((3 * P,), dev)
    mb.contact_wrench_batch(q, qd, fext=fext, cforce=cforce)
    errs = (_scaled(_np(fext), c["ref"][0]), _scaled(_np(cforce), c["ref"][1]))
    print(f"{case} contact_wrench f64: fext {errs[0]:.3e} cforce {errs[1]:.3e} (active share {share:.2f})")
    assert max(errs) <= 1e-9
    for full in (ff, fc):  # columns past the batch are untouched
        assert bool((full[:, B:] == SENTINEL).all())
    free = [6 * j + e for j in range(n) if j not in c["cm"]["links"] for e in range(6)]
    assert free and not bool(fext[free].any()), "a link without a point has a wrench"
    # outputs the binding allocates share the inputs' leading dimension
    f2, c2 = mb.contact_wrench_batch(q, qd)
    assert f2.stride(0) == LD and torch.equal(f2, fext) and torch.equal(c2, cforce)


def _rows_like(t, src):
    """t on rows of src's leading dimension."""
    out = torch.empty_strided(src.shape, src.stride(), dtype=src.dtype, device=src.device)
    return out.copy_(t)


def _composed(c, q, qd, tau_seq, dt):
    """The per-step sequence of existing entry points: contact_wrench, fd_ext, the two updates."""
    traj = []
    for tau in tau_seq:
        fext, _ = c["mb"].contact_wrench_batch(q, qd)
        a = c["plain"].fd_ext_batch(q, qd, tau, fext)
        qd = _rows_like(qd + dt * a, q)
        q = _rows_like(q + dt * qd, q)
        traj.append(q.clone())
    return torch.stack(traj), q, qd


@pytest.mark.parametrize("case", MODELS)
def test_rollout_against_composition_f64(case, dev):
    c = _case(case)
    mb, n = c["mb"], c["mb"].n
    q0, qd0, tau_seq = (_t(a, dev) for a in c["x"])
    K = tau_seq.shape[0]
    traj_ref, q_ref, qd_ref = _composed(c, q0, qd0, tau_seq, cr.DT)
    q, qd = _rows_like(q0, q0), _rows_like(qd0, q0)
    ft, traj = _padded_out((K, n), dev)
    out = mb.rollout_contact_batch(q, qd, tau_seq, cr.DT, traj=traj)
    assert out is traj and bool((ft[..., B:] == SENTINEL).all())
    errs = (_scaled(_np(traj), _np(traj_ref)), _scaled(_np(q), _np(q_ref)), _scaled(_np(qd), _np(qd_ref)))
    print(f"{case} rollout_contact f64 K={K} against the composition: traj {errs[0]:.3e} q {errs[1]:.3e} qd {errs[2]:.3e}")
    assert max(errs) <= 1e-7
    assert torch.equal(traj[-1], q)
    # the trajectory the binding allocates shares the state's leading dimension
    q2, qd2 = _t(c["x"][0], dev), _t(c["x"][1], dev)
    traj2 = mb.rollout_contact_batch(q2, qd2, tau_seq, cr.DT)
    assert traj2.stride(1) == LD and torch.equal(traj2, traj) and torch.equal(qd2, qd)


@pytest.mark.parametrize("case", ["fr3", "floating14"])
def test_rollout_against_reference_f64(case, dev):
    c = _case(case)
    mb = c["mb"]
    K = 2
    q0, qd0, tau_seq = c["x"][0], c["x"][1], c["x"][2][:K]
    traj_ref, q_ref, qd_ref, info = cr.rollout(c["om"], c["m6"], c["cm"], q0, qd0, tau_seq)
    share = cr.check_share(info)
    q, qd = _t(q0, dev), _t(qd0, dev)
    traj = mb.rollout_contact_batch(q, qd, _t(tau_seq, dev), cr.DT)
    errs = (_scaled(_np(traj), traj_ref), _scaled(_np(q), q_ref), _scaled(_np(qd), qd_ref))
    print(f"{case} rollout_contact f64 K={K} against contact_ref: traj {errs[0]:.3e} q {errs[1]:.3e} qd {errs[2]:.3e} "
          f"(active share over all steps {share:.2f})")
    assert max(errs) <= 1e-7


def test_two_handles_alternate(dev):
    """Two sets on one URDF, used alternately: each matches its own reference (the kernel cache key
    holds the set)."""
    c = _case("fr3")
    cm2 = dict(c["cm"], stiffness=3500.0, offset=c["cm"]["offset"] + 0.05, links=c["cm"]["links"][::-1])
    mb2 = c["plain"].with_contacts(cm2["links"], cm2["points"], normal=cm2["normal"], offset=cm2["offset"],
                                   stiffness=cm2["stiffness"], damping=cm2["damping"], friction=cm2["friction"],
                                   slip_velocity=cm2["slip_velocity"])
    ref2 = cr.contact_batch(c["m6"], cm2, *c["x"][:2])
    assert _scaled(ref2[0], c["ref"][0]) > 1e-3  # the two sets really differ
    q, qd = (_t(a, dev) for a in c["x"][:2])
    for _ in range(2):
        for mb, ref in ((c["mb"], c["ref"]), (mb2, ref2)):
            fext, cforce = mb.contact_wrench_batch(q, qd)
            assert max(_scaled(_np(fext), ref[0]), _scaled(_np(cforce), ref[1])) <= 1e-9


@pytest.mark.parametrize("case", MODELS)
def test_wrench_f32_against_f64_kernel(case, dev):
    c = _case(case)
    mb = c["mb"]
    q, qd = (a.astype(np.float32).astype(np.float64) for a in c["x"][:2])
    got = mb.contact_wrench_batch(_t(q, dev, torch.float32), _t(qd, dev, torch.float32))
    ref = mb.contact_wrench_batch(_t(q, dev), _t(qd, dev))
    for name, g, r in zip(("fext", "cforce"), got, ref):
        g, r = _np(g).astype(np.float64), _np(r)
        assert np.all(np.isfinite(g))
        e = np.abs(g - r).max(axis=0) / (1 + np.abs(r).max(axis=0))
        print(f"{case} contact_wrench {name} f32 norm-wise {e.max():.3e} at configuration {e.argmax()}")
        assert e.max() <= 1e-4


@pytest.mark.parametrize("case", MODELS)
def test_rollout_f32_against_f64_kernel(case, dev):
    """fp32 rollout_contact, K = 4, against the fp64 kernel on the same fp32-rounded inputs, norm-wise
    per configuration and array.  Bound 4e-4: 8x the measured maximum over the five models, 4.7e-5
    (chain16 qd; FR3 3.9e-5, general5 2.8e-5, floating14 8.9e-6, tree9 3.5e-6), rounded up."""
    c = _case(case)
    mb = c["mb"]
    q, qd, tau_seq = (a.astype(np.float32).astype(np.float64) for a in c["x"])
    outs = []
    for dtype in (torch.float32, torch.float64):
        tq, tqd = _t(q, dev, dtype), _t(qd, dev, dtype)
        traj = mb.rollout_contact_batch(tq, tqd, _t(tau_seq, dev, dtype), cr.DT)
        outs.append([_np(t).astype(np.float64) for t in (traj, tq, tqd)])
    worst = 0.0
    for name, g, r in zip(("traj", "q", "qd"), *outs):
        assert np.all(np.isfinite(g)), name
        g, r = g.reshape(-1, B), r.reshape(-1, B)
        e = np.abs(g - r).max(axis=0) / (1 + np.abs(r).max(axis=0))
        worst = max(worst, e.max())
        print(f"{case} rollout_contact {name} f32 K=4 norm-wise {e.max():.3e} at configuration {e.argmax()}")
    assert worst <= 4e-4


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", ["fr3", "tree9"])
def test_input_domain(case, dtype, dev):
    """fp32 too: there the outputs, and the wrench the dynamics check, reach the guard's inline assembly
    through a wait state of their own -- a stale register read would show as a missing NaN."""
    c = _case(case)
    mb, n = c["mb"], c["mb"].n
    q, qd, tau_seq = (_t(a, dev, dtype) for a in c["x"])
    keep = np.ones(B, bool)
    keep[17] = False

    def run(qb, qdb, tb):
        fext, cforce = mb.contact_wrench_batch(qb, qdb)
        rq, rqd = _t(_np(qb), dev, dtype), _t(_np(qdb), dev, dtype)
        traj = mb.rollout_contact_batch(rq, rqd, tb, cr.DT)
        return [_np(t) for t in (fext, cforce, traj.reshape(-1, B), rq, rqd)]

    clean = run(q, qd, tau_seq)
    assert all(np.isfinite(a).all() for a in clean)
    for which, row, bad in (("q", 1, float("nan")), ("q", n - 1, float("nan")), ("qd", 2, float("inf"))):
        qb, qdb = q.clone(), qd.clone()
        (qb if which == "q" else qdb)[row, 17] = bad
        for k, (got, ref) in enumerate(zip(run(qb, qdb, tau_seq), clean)):
            assert np.isnan(got[:, 17]).all(), (which, row, k)
            assert np.array_equal(got[:, keep], ref[:, keep]), (which, row, k)
    # a NaN torque at step 1: step 0 is clean, everything from step 1 on is NaN
    tb = _t(c["x"][2], dev, dtype)
    tb[1, n // 2, 17] = float("nan")
    rq, rqd = _t(c["x"][0], dev, dtype), _t(c["x"][1], dev, dtype)
    traj = _np(mb.rollout_contact_batch(rq, rqd, tb, cr.DT))
    ctraj = clean[2].reshape(traj.shape)
    assert np.array_equal(traj[0], ctraj[0])
    assert np.isnan(traj[1:, :, 17]).all() and np.isnan(_np(rq)[:, 17]).all() and np.isnan(_np(rqd)[:, 17]).all()
    assert np.array_equal(traj[:, :, keep], ctraj[:, :, keep])
    assert np.array_equal(_np(rq)[:, keep], clean[3][:, keep])


@pytest.mark.parametrize("batch", [1, 256])
def test_batch_edges(batch, dev):
    c = _case("fr3")
    mb = c["mb"]
    q, qd = (torch.as_tensor(np.ascontiguousarray(a[:, :batch]), device=dev) for a in c["x"][:2])
    tau_seq = torch.as_tensor(np.ascontiguousarray(c["x"][2][:, :, :batch]), device=dev)
    fext, cforce = mb.contact_wrench_batch(q, qd)
    assert _scaled(_np(fext), c["ref"][0][:, :batch]) <= 1e-9 and _scaled(_np(cforce), c["ref"][1][:, :batch]) <= 1e-9
    traj_ref, q_ref, qd_ref = _composed(c, q, qd, tau_seq, cr.DT)
    traj = mb.rollout_contact_batch(q, qd, tau_seq, cr.DT)
    assert traj.shape == tau_seq.shape
    assert max(_scaled(_np(traj), _np(traj_ref)), _scaled(_np(q), _np(q_ref)), _scaled(_np(qd), _np(qd_ref))) <= 1e-7


def test_host_pointer_forms_equal_device_forms(dev):
    c = _case("tree9")
    mb = c["mb"]
    q, qd, tau_seq = c["x"]
    for npd, dtype in ((np.float64, torch.float64), (np.float32, torch.float32)):
        tq, tqd = _t(q, dev, dtype), _t(qd, dev, dtype)
        fext, cforce = mb.contact_wrench_batch_host(q, qd, dtype=npd)
        dfext, dcforce = mb.contact_wrench_batch(tq, tqd)
        assert np.array_equal(fext, _np(dfext)) and np.array_equal(cforce, _np(dcforce))
        traj, qk, qdk = mb.rollout_contact_batch_host(q, qd, tau_seq, cr.DT, dtype=npd)
        dtraj = mb.rollout_contact_batch(tq, tqd, _t(tau_seq, dev, dtype), cr.DT)
        assert np.array_equal(traj, _np(dtraj)) and np.array_equal(qk, _np(tq)) and np.array_equal(qdk, _np(tqd))


def test_without_hiprtc_fails_loudly(dev):
    from rigidbody_amd import ffi

    c = _case("fr3")
    mb = c["plain"].with_contacts([6], [[0.0, 0.0, 0.1]], offset=0.25, stiffness=1234.0)  # kernels not built yet
    z = torch.zeros((mb.n, 8), dtype=torch.float64, device=dev)
    try:
        ffi.set_tuning("jit", 0)
        with pytest.raises(ffi.RigidBodyError, match="hipRTC"):
            mb.contact_wrench_batch(z, z)
        with pytest.raises(ffi.RigidBodyError, match="hipRTC"):
            mb.rollout_contact_batch(z.clone(), z.clone(), torch.zeros((2, mb.n, 8), dtype=torch.float64, device=dev), 1e-3)
    finally:
        ffi.set_tuning("jit", 1)
