"""Kinematics of every link without a GPU: the single-configuration host forms multibody_link_pose /
multibody_link_vel (the kernels' lane bodies compiled for the host, link_kin_body.hip.hpp), the
hipRTC compile of every kernel form, and the argument checks the new entry points add.  Reference:
tests/link_kin_ref.py (world poses and link velocities composed from the 6x6 model's own joint
transforms); bounds are the header's fp64 contracts."""
import ctypes

import numpy as np
import pytest

import ext_wrench_ref as xr
import link_kin_ref as lk

ARG, UNSUPPORTED = 2, 6  # rb_status


@pytest.fixture(scope="module")
def ffi():
    from rigidbody_amd import ffi

    if not hasattr(ffi.Multibody, "link_pose"):
        pytest.fail("the binding has no link-kinematics entry points")
    return ffi


def _scaled(got, ref):
    return (np.abs(np.asarray(got).reshape(-1) - ref) / (1.0 + np.abs(ref))).max()


@pytest.mark.parametrize("case", ["fr3", "chain12", "chain16", "chain30"])
def test_single_configuration_against_reference(ffi, case):
    mb, om, m6 = xr.setup(case)
    n = mb.n
    q, qd = xr.inputs(mb, 8, 51)[:2]
    worst = 0.0
    for b in range(q.shape[1]):
        pos_ref, rot_ref, vel_ref = lk.link_kin(m6, q[:, b], qd[:, b])
        pos, rot = mb.link_pose(q[:, b])
        vel = mb.link_vel(q[:, b], qd[:, b])
        assert pos.shape == (n, 3) and rot.shape == (n, 3, 3) and vel.shape == (n, 6)
        errs = (_scaled(pos, pos_ref), _scaled(rot.transpose(0, 2, 1), rot_ref), _scaled(vel, vel_ref))
        worst = max(worst, *errs)
        assert max(errs) <= 1e-9, (case, b, errs)
        # the last link is what the reference's two queries report
        fk = mb.fwd_kin(q[:, b])
        assert _scaled(pos[n - 1], fk) <= 1e-12, (case, b)
        jv = qd[:, b] @ mb.jac_raw(q[:, b]).reshape(n, 6)  # column j of the 6 x n Jacobian, rows [lin; rot]
        assert _scaled(vel[n - 1], jv) <= 1e-12, (case, b)
        eye = np.einsum("jab,jcb->jac", rot, rot)
        assert np.abs(eye - np.eye(3)).max() <= 1e-12, (case, b)
    print(f"{case} link_pose / link_vel host f64 {worst:.3e}")


def test_position_is_the_oracle_fwd_kin_of_the_truncated_chain(ffi):
    """Link j of a serial chain is the last link of the chain cut after it: its position is what the
    oracle's own fwd_kin gives for the leading joints (an independent check of the reference)."""
    mb, om, m6 = xr.setup("fr3")
    q, qd = xr.inputs(mb, 4, 52)[:2]
    for b in range(q.shape[1]):
        pos_ref, _, _ = lk.link_kin(m6, q[:, b], qd[:, b])
        assert np.abs(pos_ref[-3:] - om.fwd_kin(q[:, b])).max() <= 1e-12
        assert np.abs(pos_ref[-3:] - m6.fwd_kin(q[:, b])).max() <= 1e-12


CASES = ["fr3", "general5", "tree9", "floating14"]


@pytest.mark.parametrize("case", CASES)
def test_kernels_compile_for_gfx950(ffi, case):
    """hipRTC needs no device: every form (link_pose / link_vel, fp32 / fp64) builds for gfx950 and
    calls the new lane function."""
    mb, _, _ = xr.setup(case)
    for vel, lane in ((0, "link_pose_lane"), (1, "link_vel_lane")):
        for f64 in (0, 1):
            assert mb.link_kin_jit_compile(vel, f64, "gfx950") > 0, (case, vel, f64)
            src = mb.link_kin_jit_source(vel, f64)
            assert src and "rbamd::dev::" + lane in src and "kExtRa" in src, (case, vel, f64)


def test_alias_refusals(ffi):
    lib, mb = ffi.lib(), ffi.Multibody.new()
    bufs = [(ctypes.c_double * 64)() for _ in range(3)]
    p = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    d = [ctypes.cast(b, ctypes.POINTER(ctypes.c_double)) for b in bufs]
    for t in ("f32", "f64"):
        pose, vel = getattr(lib, f"multibody_link_pose_batch_{t}"), getattr(lib, f"multibody_link_vel_batch_{t}")
        assert pose(mb.handle, p[0], p[0], p[2], 1, 1, None) == ARG
        assert ffi.last_error() == "link_pose: an output array is also an input"
        assert pose(mb.handle, p[0], p[1], p[0], 1, 1, None) == ARG
        assert pose(mb.handle, p[0], p[1], p[1], 1, 1, None) == ARG
        assert ffi.last_error() == "link_pose: two outputs are the same array"
        for i in range(2):
            assert vel(mb.handle, p[0], p[1], p[i], 1, 1, None) == ARG, i
            assert ffi.last_error() == "link_vel: an output array is also an input"
    assert lib.multibody_link_pose(mb.handle, d[0], d[0], d[1]) == ARG
    assert lib.multibody_link_pose(mb.handle, d[0], d[1], d[1]) == ARG
    assert lib.multibody_link_vel(mb.handle, d[0], d[1], d[1]) == ARG
    assert ffi.last_error().startswith("link_vel:")


@pytest.mark.parametrize("case", ["tree9", "floating14"])
def test_single_configuration_form_refuses_trees(ffi, case):
    mb, _, _ = xr.setup(case)
    z = np.zeros(mb.n)
    with pytest.raises(ffi.RigidBodyError, match="serial revolute"):
        mb.link_pose(z)
    with pytest.raises(ffi.RigidBodyError, match="serial revolute"):
        mb.link_vel(z, z)
    dp = ctypes.POINTER(ctypes.c_double)
    out = np.zeros(9 * mb.n)
    assert ffi.lib().multibody_link_vel(mb.handle, z.ctypes.data_as(dp), np.zeros(mb.n).ctypes.data_as(dp),
                                        out.ctypes.data_as(dp)) == UNSUPPORTED
