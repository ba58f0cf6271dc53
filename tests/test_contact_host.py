"""Compliant ground contact without a GPU: the single-configuration host forms
multibody_contact_wrench / multibody_rollout_contact (the kernels' lane bodies compiled for the host,
contact_body.hip.hpp), the handle that carries a contact set (refusals, getter, blob), the argument
checks of every new entry point, and the hipRTC compile of every kernel form.  Reference:
tests/contact_ref.py (the header's law on link_kin_ref, the oracle's forward dynamics under the
wrench); bounds are the header's fp64 contracts."""
import ctypes

import numpy as np
import pytest

import contact_ref as cr
import ext_wrench_ref as xr
import link_kin_ref as lk

NULL, ARG, UNSUPPORTED = 1, 2, 6  # rb_status
B = 257  # the GPU tests' batch: the reference's clipped branch needs that many configurations on FR3
BR = 48  # configurations of the rollout tests (their own batch: the plane sits at its median height)


@pytest.fixture(scope="module")
def ffi():
    from rigidbody_amd import ffi

    if not hasattr(ffi.Multibody, "with_contacts"):
        pytest.fail("the binding has no contact entry points")
    return ffi


def _scaled(got, ref):
    got, ref = np.asarray(got, float).reshape(-1), np.asarray(ref, float).reshape(-1)
    assert np.all(np.isfinite(got))
    return (np.abs(got - ref) / (1.0 + np.abs(ref))).max()


_cache = {}


def _case(case, batch=B):
    if (case, batch) not in _cache:
        _cache[case, batch] = cr.setup(case, batch, 71)
    return _cache[case, batch]


@pytest.mark.parametrize("case", ["fr3", "chain16", "chain30"])
def test_contact_wrench_against_reference(ffi, case):
    mb, _, om, m6, cm, (q, qd, _) = _case(case)
    fext_ref, cforce_ref, info = cr.contact_batch(m6, cm, q, qd)
    share = cr.check_share(info)
    worst = 0.0
    for b in range(B):
        fext, cforce = mb.contact_wrench(q[:, b], qd[:, b])
        assert fext.shape == (mb.n, 6) and cforce.shape == (len(cm["links"]), 3)
        errs = (_scaled(fext, fext_ref[:, b]), _scaled(cforce, cforce_ref[:, b]))
        worst = max(worst, *errs)
        assert max(errs) <= 1e-9, (case, b, errs)
        rows = fext[[j for j in range(mb.n) if j not in cm["links"]]]
        assert not rows.any(), "a link without a point has a wrench"
    print(f"{case} contact_wrench host f64 {worst:.3e} (active share {share:.2f})")


@pytest.mark.parametrize("case", ["fr3", "chain16", "chain30"])
def test_rollout_contact_against_reference(ffi, case):
    mb, _, om, m6, cm, (q, qd, tau) = _case(case, BR)
    K = 3
    rng = np.random.default_rng(72)
    tau_seq = np.stack([tau[:, rng.permutation(BR)] for _ in range(K)])
    traj_ref, q_ref, qd_ref, info = cr.rollout(om, m6, cm, q, qd, tau_seq)
    share = cr.check_share(info)
    worst = 0.0
    for b in range(BR):
        q0, qd0 = q[:, b].copy(), qd[:, b].copy()
        traj, qk, qdk = mb.rollout_contact(q0, qd0, tau_seq[:, :, b], cr.DT)
        assert np.array_equal(q0, q[:, b]) and np.array_equal(traj[-1], qk)
        errs = (_scaled(traj, traj_ref[:, :, b]), _scaled(qk, q_ref[:, b]), _scaled(qdk, qd_ref[:, b]))
        worst = max(worst, *errs)
        assert max(errs) <= 1e-7, (case, b, errs)
    print(f"{case} rollout_contact host f64 K={K} {worst:.3e} (active share over all steps {share:.2f})")


@pytest.mark.parametrize("case", ["fr3", "chain16"])
def test_power_identity(ffi, case):
    """sum_p F_p . xd_p == sum_j fext_j . vel_j, vel from multibody_link_vel: cforce, fext and the
    link kinematics agree on frames and row order."""
    mb, _, om, m6, cm, (q, qd, _) = _case(case)
    worst = 0.0
    for b in range(BR):
        fext, cforce = mb.contact_wrench(q[:, b], qd[:, b])
        vel = mb.link_vel(q[:, b], qd[:, b])
        _, xd, _ = cr.point_kin(m6, cm["links"], cm["points"], q[:, b], qd[:, b])
        lhs, per_link = (cforce * xd).sum(), (fext * vel).sum(axis=1)
        err = abs(lhs - per_link.sum()) / (1.0 + np.abs(per_link).sum())
        worst = max(worst, err)
        assert err <= 1e-8, (case, b, err)
    print(f"{case} contact power identity {worst:.3e}")


def test_frictionless_force_is_normal(ffi):
    mb, _, om, m6, cm, (q, qd, _) = cr.setup("fr3", BR, 71, friction=0.0, normal=(0.6, 0.0, 0.8))
    nh = np.array(cm["normal"])
    active = 0
    for b in range(BR):
        _, cforce = mb.contact_wrench(q[:, b], qd[:, b])
        assert np.abs(np.cross(cforce, nh)).max() <= 1e-12 * (1.0 + np.abs(cforce).max())
        assert (cforce @ nh >= 0).all()
        active += int((cforce @ nh > 0).sum())
    assert active > 0


def test_no_contact(ffi):
    """The plane below every point: exact zeros, and the rollout is the contact-free step."""
    mb, plain, om, m6, cm, (q, qd, tau) = cr.setup("fr3", 8, 73, offset=-100.0)
    for b in range(8):
        fext, cforce = mb.contact_wrench(q[:, b], qd[:, b])
        assert not fext.any() and not cforce.any()
        traj, qk, qdk = mb.rollout_contact(q[:, b], qd[:, b], tau[None, :, b], cr.DT)
        a = plain.fd_ext(q[:, b], qd[:, b], tau[:, b], np.zeros(6 * mb.n))
        qd_ref = qd[:, b] + cr.DT * a
        q_ref = q[:, b] + cr.DT * qd_ref
        assert _scaled(qdk, qd_ref) <= 1e-12 and _scaled(qk, q_ref) <= 1e-12 and _scaled(traj[0], q_ref) <= 1e-12


def test_with_contacts_refusals(ffi):
    mb = ffi.Multibody.new()
    ok = dict(links=[6, 3], points=[[0, 0, 0.1], [0.1, 0, 0]], normal=(0, 0, 1), offset=0.2, stiffness=1e3, damping=0.1,
              friction=0.5, slip_velocity=0.01)
    assert mb.with_contacts(**ok).n_contacts == 2
    nan, inf = float("nan"), float("inf")
    bad = [
        (dict(links=[], points=np.zeros((0, 3))), "n_points"),
        (dict(links=[0] * 17, points=np.zeros((17, 3))), "n_points"),
        (dict(links=[7, 3]), "link[0]"),
        (dict(links=[6, -1]), "link[1]"),
        (dict(points=[[0, 0, 0.1], [nan, 0, 0]]), "point[1]"),
        (dict(normal=(0, inf, 1)), "normal"),
        (dict(normal=(0, 0, 1.001)), "normal"),
        (dict(normal=(0, 0, 0)), "normal"),
        (dict(offset=nan), "offset"),
        (dict(stiffness=-1.0), "stiffness"),
        (dict(stiffness=inf), "stiffness"),
        (dict(damping=-0.1), "damping"),
        (dict(friction=-0.5), "friction"),
        (dict(friction=nan), "friction"),
        (dict(slip_velocity=0.0), "slip_velocity"),
        (dict(slip_velocity=-1.0), "slip_velocity"),
    ]
    for change, field in bad:
        with pytest.raises(ffi.RigidBodyError) as e:
            mb.with_contacts(**{**ok, **change})
        assert field in str(e.value), (change, str(e.value))
    assert mb.with_contacts(**{**ok, "normal": (0, 0, 1 + 5e-7)}).n_contacts == 2
    assert not ffi.lib().multibody_with_contacts(None, None) and ffi.last_error() == "NULL Multibody handle"
    assert not ffi.lib().multibody_with_contacts(mb.handle, None)
    assert mb.n_contacts == 0 and mb.contact_model() is None  # the source handle is not modified


def test_getter_round_trip(ffi):
    mb, _, _, _, cm, _ = _case("fr3")
    got = mb.contact_model()
    assert got["links"] == cm["links"] and np.array_equal(got["points"], cm["points"])
    assert got["normal"] == tuple(cm["normal"]) and got["offset"] == cm["offset"]
    for k in cr.PARAMS:
        assert got[k] == cm[k], k
    assert ffi.lib().multibody_contact_model(None, None) == -NULL


def test_blob_carries_the_set(ffi):
    mb, plain, _, _, cm, (q, qd, _) = _case("fr3")
    pb, cb = plain.blob(), mb.blob()
    assert len(pb) == 5 + 38 * mb.n, "the blob of a model without a contact set has changed length"
    assert len(cb) == len(pb) + 9 + 4 * len(cm["links"]) and np.array_equal(cb[:len(pb)], pb)
    again = ffi.Multibody.from_blob(cb)
    got = again.contact_model()
    assert got["links"] == cm["links"] and np.array_equal(got["points"], cm["points"]) and got["offset"] == cm["offset"]
    assert np.array_equal(again.blob(), cb)
    a, b = mb.contact_wrench(q[:, 0], qd[:, 0]), again.contact_wrench(q[:, 0], qd[:, 0])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert ffi.Multibody.from_blob(pb).n_contacts == 0 and np.array_equal(ffi.Multibody.from_blob(pb).blob(), pb)
    for broken in (cb[:-1], np.append(cb, 0.0)):
        with pytest.raises(ffi.RigidBodyError):
            ffi.Multibody.from_blob(broken)
    bad = cb.copy()
    bad[len(pb) + 1] = 99.0  # the first point's link
    with pytest.raises(ffi.RigidBodyError, match="link"):
        ffi.Multibody.from_blob(bad)


def _names(lib):
    for t in ("f32", "f64"):
        for form in ("", "_host"):
            yield (getattr(lib, f"multibody_contact_wrench_batch{form}_{t}"),
                   getattr(lib, f"multibody_rollout_contact_batch{form}_{t}"), form == "")


def test_model_without_a_set_is_refused(ffi):
    lib, mb = ffi.lib(), ffi.Multibody.new()
    p = [ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p) for _ in range(4)]
    for wrench, rollout, dev in _names(lib):
        tail = (1, 1, None) if dev else (1,)
        assert wrench(mb.handle, *p, *tail) == UNSUPPORTED
        assert "multibody_with_contacts" in ffi.last_error()
        assert rollout(mb.handle, p[0], p[1], p[2], 1e-3, 2, p[3], *tail) == UNSUPPORTED
        assert "multibody_with_contacts" in ffi.last_error()
        assert rollout(mb.handle, p[0], p[1], p[2], 1e-3, 0, p[3], *tail) == 0  # K == 0: nothing looked at
        assert rollout(mb.handle, p[0], p[1], p[2], 1e-3, -1, p[3], *tail) == ARG
        assert ffi.last_error() == "negative step count"
    z = np.zeros(mb.n)
    with pytest.raises(ffi.RigidBodyError, match="multibody_with_contacts"):
        mb.contact_wrench(z, z)
    with pytest.raises(ffi.RigidBodyError, match="multibody_with_contacts"):
        mb.rollout_contact(z, z, z[None], 1e-3)
    for rollout in (0, 1):
        assert mb.contact_jit_source(rollout, 1) == ""
        assert lib.multibody_contact_jit_compile(mb.handle, rollout, 1, 1 << 20, None) == -UNSUPPORTED
        assert lib.multibody_contact_jit_compile(None, rollout, 1, 1 << 20, None) == -NULL
        assert lib.multibody_contact_jit_compile(mb.handle, rollout, 1, 0, None) == -ARG


def test_alias_refusals(ffi):
    lib = ffi.lib()
    mb = _case("fr3")[0]
    p = [ctypes.cast((ctypes.c_double * 64)(), ctypes.c_void_p) for _ in range(4)]
    for wrench, rollout, dev in _names(lib):
        tail = (1, 1, None) if dev else (1,)
        for out in ((p[0], p[3]), (p[2], p[1])):
            assert wrench(mb.handle, p[0], p[1], *out, *tail) == ARG
            assert ffi.last_error() == "contact_wrench: an output array is also an input"
        assert wrench(mb.handle, p[0], p[1], p[2], p[2], *tail) == ARG
        assert ffi.last_error() == "contact_wrench: two outputs are the same array"
        assert rollout(mb.handle, p[0], p[1], p[2], 1e-3, 1, p[2], *tail) == ARG
        assert ffi.last_error() == "rollout_contact: an output array is also an input"
        assert rollout(mb.handle, p[0], p[2], p[2], 1e-3, 1, p[3], *tail) == ARG
        for args in ((p[0], p[0], p[2], p[3]), (p[0], p[1], p[2], p[0]), (p[0], p[1], p[2], p[1])):
            assert rollout(mb.handle, *args[:3], 1e-3, 1, args[3], *tail) == ARG, args
            assert ffi.last_error() == "rollout_contact: two outputs are the same array"
        assert wrench(mb.handle, p[0], p[0], None, p[0], *tail) == NULL  # NULL arrays first
    d = [ctypes.cast(x, ctypes.POINTER(ctypes.c_double)) for x in p]
    assert lib.multibody_contact_wrench(mb.handle, d[0], d[1], d[1], d[2]) == ARG
    assert lib.multibody_contact_wrench(mb.handle, d[0], d[1], d[2], None) == NULL
    assert lib.multibody_rollout_contact(mb.handle, d[0], d[1], d[2], 1e-3, 1, d[0]) == ARG
    assert lib.multibody_rollout_contact(mb.handle, d[0], d[1], d[2], 1e-3, -1, d[3]) == ARG
    assert lib.multibody_rollout_contact(mb.handle, None, None, None, 1e-3, 0, None) == 0


@pytest.mark.parametrize("case", ["tree9", "floating14"])
def test_single_configuration_form_refuses_trees(ffi, case):
    mb = cr.setup(case, 4, 74)[0]
    z = np.zeros(mb.n)
    with pytest.raises(ffi.RigidBodyError, match="serial revolute"):
        mb.contact_wrench(z, z)
    with pytest.raises(ffi.RigidBodyError, match="serial revolute"):
        mb.rollout_contact(z, z, z[None], 1e-3)


def test_two_handles_have_their_own_source(ffi):
    plain = ffi.Multibody.new()
    a = plain.with_contacts([6], [[0, 0, 0.1]], offset=0.3, stiffness=2000.0)
    b = plain.with_contacts([6], [[0, 0, 0.1]], offset=0.3, stiffness=2500.0)
    c = plain.with_contacts([6, 2], [[0, 0, 0.1], [0, 0, 0.1]], offset=0.3, stiffness=2000.0)
    for rollout in (0, 1):
        srcs = [m.contact_jit_source(rollout, 1) for m in (a, b, c)]
        assert all(srcs) and len(set(srcs)) == 3
        assert "2500.0" in srcs[1] and "2500.0" not in srcs[0]
    # mu == 0 is a constant too
    assert a.contact_jit_source(0, 0) != plain.with_contacts([6], [[0, 0, 0.1]], offset=0.3, friction=0.0).contact_jit_source(0, 0)


@pytest.mark.parametrize("case", ["fr3", "general5", "tree9", "floating14"])
def test_kernels_compile_for_gfx950(ffi, case):
    """hipRTC needs no device: every form (contact_wrench / rollout_contact, fp32 / fp64) builds for
    gfx950 and calls the new lane function with the set compiled in."""
    mb = cr.setup(case, 4, 75)[0]
    for rollout, lane in ((0, "contact_wrench_lane"), (1, "rollout_contact_lane")):
        for f64 in (0, 1):
            assert mb.contact_jit_compile(rollout, f64, "gfx950") > 0, (case, rollout, f64)
            src = mb.contact_jit_source(rollout, f64)
            assert "rbamd::dev::" + lane in src and "struct Con" in src and "kExtRa" in src, (case, rollout, f64)
