"""Kinematics of every link on the GPU: multibody_link_pose_batch_* / multibody_link_vel_batch_*
against tests/link_kin_ref.py (world poses and link velocities composed from the 6x6 model's own
joint transforms).  Every batch is B = 257 -- one full 256-lane block and a one-lane tail -- on rows
of leading dimension 300.  Bounds: the header's (fp64 1e-9 scaled, the fwd_kin / jac contract; the
power identity with the external-wrench kernels 1e-8; fp32 1e-4 norm-wise, the rnea_ext contract).

Measured on MI355X (this file's own prints): fp64 against the reference 9.3e-16 FR3, 2.1e-15 16
links, 1.8e-15 general5, 1.8e-15 tree9, 2.6e-15 floating14 (the largest is vel each time); power
identity 1.1e-15 at most (floating14); fp32 against the fp64 kernel 2.7e-7 at most (floating14
link_vel); |q| ~ 2^40 1.4e-15."""
import numpy as np
import pytest

import ext_wrench_ref as xr
import link_kin_ref as lk

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

    if not hasattr(ffi.Multibody, "link_pose_batch"):
        pytest.fail("the binding has no link-kinematics entry points")
    return torch.device("cuda:0")


def _case(case):
    """Model, inputs and reference of one case, computed once and never modified."""
    if case not in _cache:
        mb, om, m6 = xr.setup(case)
        q, qd, qdd, _, fext = xr.inputs(mb, B, 61)
        ref = lk.link_kin_batch(m6, q, qd)
        _cache[case] = dict(mb=mb, m6=m6, x=(q, qd, qdd, fext), ref=ref)
        for a in (q, qd, qdd, fext, *ref):
            a.setflags(write=False)
    return _cache[case]


def _t(a, dev, dtype=torch.float64, fill=0.0):
    """[rows, B] view of a [rows, LD] device tensor whose padding columns hold `fill`."""
    a = np.array(a)  # a writable copy: the cached inputs are read-only
    t = torch.full((a.shape[0], LD), fill, dtype=dtype, device=dev)
    t[:, :B] = torch.as_tensor(a, dtype=dtype, device=dev)
    return t[:, :B]


def _padded_out(rows, dev, dtype=torch.float64):
    full = torch.full((rows, LD), SENTINEL, dtype=dtype, device=dev)
    return full, full[:, :B]


def _scaled(got, ref):
    got = np.asarray(got, float)
    assert np.all(np.isfinite(got)), "non-finite output"
    return (np.abs(got - ref) / (1.0 + np.abs(ref))).max()


@pytest.mark.parametrize("case", MODELS)
def test_parity_f64(case, dev):
    c = _case(case)
    mb, n = c["mb"], c["mb"].n
    q, qd = (_t(a, dev) for a in c["x"][:2])
    assert q.stride(0) == LD
    (fp, pos), (fr, rot), (fv, vel) = (_padded_out(r * n, dev) for r in (3, 9, 6))
    mb.link_pose_batch(q, pos=pos, rot=rot)
    mb.link_vel_batch(q, qd, out=vel)
    errs = [_scaled(t.cpu().numpy(), r) for t, r in zip((pos, rot, vel), c["ref"])]
    print(f"{case} link_pose / link_vel f64: pos {errs[0]:.3e} rot {errs[1]:.3e} vel {errs[2]:.3e}")
    assert max(errs) <= 1e-9
    for full in (fp, fr, fv):  # columns past the batch are untouched
        assert bool((full[:, B:] == SENTINEL).all())
    # outputs the binding allocates share the inputs' leading dimension
    pos2, rot2 = mb.link_pose_batch(q)
    assert pos2.stride(0) == LD and torch.equal(pos2, pos) and torch.equal(rot2, rot)
    assert torch.equal(mb.link_vel_batch(q, qd), vel)


@pytest.mark.parametrize("case", ["fr3", "general5", "tree9", "floating14"])
def test_power_identity_with_the_wrench_kernels(case, dev):
    """vel and fext share frame and row order: sum_j fext_j . vel_j = qd^T (rnea - rnea_ext) = qd^T
    sum_j J_j^T fext_j, per configuration."""
    c = _case(case)
    mb, n = c["mb"], c["mb"].n
    q, qd, qdd, fext = (_t(a, dev) for a in c["x"])
    vel = mb.link_vel_batch(q, qd).cpu().numpy()
    d = (mb.rnea_batch(q, qd, qdd) - mb.rnea_ext_batch(q, qd, qdd, fext)).cpu().numpy()
    per_link = (c["x"][3] * vel).reshape(n, 6, B).sum(axis=1)
    lhs, rhs = per_link.sum(axis=0), (c["x"][1] * d).sum(axis=0)
    err = (np.abs(lhs - rhs) / (1.0 + np.abs(per_link).sum(axis=0))).max()
    print(f"{case} power identity {err:.3e}")
    assert err <= 1e-8


@pytest.mark.parametrize("case", ["fr3", "general5", "tree9", "floating14"])
def test_f32_against_f64_kernel(case, dev):
    c = _case(case)
    mb = c["mb"]
    q, qd = (a.astype(np.float32).astype(np.float64) for a in c["x"][:2])
    q32, qd32 = _t(q, dev, torch.float32), _t(qd, dev, torch.float32)
    q64, qd64 = _t(q, dev), _t(qd, dev)
    got = (*mb.link_pose_batch(q32), mb.link_vel_batch(q32, qd32))
    ref = (*mb.link_pose_batch(q64), mb.link_vel_batch(q64, qd64))
    for name, g, r in zip(("pos", "rot", "vel"), got, ref):
        g, r = g.cpu().numpy().astype(np.float64), r.cpu().numpy()
        assert np.all(np.isfinite(g))
        e = np.abs(g - r).max(axis=0) / (1 + np.abs(r).max(axis=0))
        print(f"{case} {name} f32 norm-wise {e.max():.3e} at configuration {e.argmax()}")
        assert e.max() <= 1e-4


@pytest.mark.parametrize("case", ["fr3", "tree9"])
def test_input_domain(case, dev):
    c = _case(case)
    mb = c["mb"]
    q, qd = (_t(a, dev) for a in c["x"][:2])
    clean = (*mb.link_pose_batch(q), mb.link_vel_batch(q, qd))
    keep = np.ones(B, bool)
    keep[17] = False
    for which, row, bad in (("q", 1, float("nan")), ("q", mb.n - 1, float("nan")), ("qd", 2, float("inf"))):
        qb, qdb = q.clone(), qd.clone()
        (qb if which == "q" else qdb)[row, 17] = bad
        outs = (*mb.link_pose_batch(qb), mb.link_vel_batch(qb, qdb))
        for k, (got, ref) in enumerate(zip(outs, clean)):
            got, ref = got.cpu().numpy(), ref.cpu().numpy()
            if which == "q" or k == 2:  # qd is no input of link_pose
                assert np.isnan(got[:, 17]).all(), (which, row, k)
            else:
                assert np.array_equal(got[:, 17], ref[:, 17]), (which, row, k)
            assert np.array_equal(got[:, keep], ref[:, keep]), (which, row, k)


def test_large_angles_f64(dev):
    """FR3, |q| ~ 2^40 rad: against the reference evaluated at the reduced angle (the sine and cosine
    of the full angle are exact in the C library; the reduced angle is their atan2), to the fp64
    bound tests/test_gpu_domain.py holds fwd_kin / jac to there."""
    c = _case("fr3")
    mb, m6 = c["mb"], c["m6"]
    rng = np.random.default_rng(62)
    q = rng.choice([-1.0, 1.0], (mb.n, B)) * 2.0 ** 40 + rng.uniform(-np.pi, np.pi, (mb.n, B))
    qd = c["x"][1]
    ref = lk.link_kin_batch(m6, np.arctan2(np.sin(q), np.cos(q)), qd)
    tq, tqd = _t(q, dev), _t(qd, dev)
    got = (*mb.link_pose_batch(tq), mb.link_vel_batch(tq, tqd))
    err = max(_scaled(g.cpu().numpy(), r) for g, r in zip(got, ref))
    print(f"fr3 |q| ~ 2^40 link_pose / link_vel f64 {err:.3e}")
    assert err <= 1e-9


def test_host_pointer_forms_equal_device_forms(dev):
    c = _case("tree9")
    mb = c["mb"]
    q, qd = c["x"][:2]
    for npd, dtype in ((np.float64, torch.float64), (np.float32, torch.float32)):
        tq, tqd = _t(q, dev, dtype), _t(qd, dev, dtype)
        pos, rot = mb.link_pose_batch_host(q, dtype=npd)
        dpos, drot = mb.link_pose_batch(tq)
        assert np.array_equal(pos, dpos.cpu().numpy()) and np.array_equal(rot, drot.cpu().numpy())
        assert np.array_equal(mb.link_vel_batch_host(q, qd, dtype=npd), mb.link_vel_batch(tq, tqd).cpu().numpy())


def test_without_hiprtc_fails_loudly(dev):
    from rigidbody_amd import ffi

    mb = _case("fr3")["mb"]
    z = torch.zeros((mb.n, 8), dtype=torch.float64, device=dev)
    try:
        ffi.set_tuning("jit", 0)
        with pytest.raises(ffi.RigidBodyError, match="hipRTC"):
            mb.link_pose_batch(z)
        with pytest.raises(ffi.RigidBodyError, match="hipRTC"):
            mb.link_vel_batch(z, z)
    finally:
        ffi.set_tuning("jit", 1)
