"""Centre of mass, centroidal momentum / energy and the centroidal momentum matrix without a GPU: the
single-configuration host forms multibody_com / multibody_centroidal / multibody_cmm (the kernels'
lane bodies compiled for the host, centroidal_body.hip.hpp), the hipRTC compile of every kernel form,
and the argument checks the new entry points add.  Reference: tests/centroidal_ref.py (the header's
definitions on the 6x6 model's own joint transforms and link inertias); bounds are the header's fp64
contracts."""
import ctypes

import numpy as np
import pytest

import centroidal_ref as cz
import ext_wrench_ref as xr

ARG, UNSUPPORTED = 2, 6  # rb_status
G = 9.81


@pytest.fixture(scope="module")
def ffi():
    from rigidbody_amd import ffi

    if not hasattr(ffi.Multibody, "centroidal"):
        pytest.fail("the binding has no centroidal entry points")
    return ffi


def _scaled(got, ref):
    ref = np.asarray(ref, float).reshape(-1)
    return (np.abs(np.asarray(got, float).reshape(-1) - ref) / (1.0 + np.abs(ref))).max()


@pytest.mark.parametrize("case", ["fr3", "chain12", "chain30", "general7"])
def test_single_configuration_against_reference(ffi, case):
    mb, om, m6 = xr.setup(case)
    n = mb.n
    q, qd = xr.inputs(mb, 6, 71)[:2]
    assert abs(mb.total_mass - cz.total_mass(m6)) <= 1e-12 * mb.total_mass
    worst = 0.0
    for b in range(q.shape[1]):
        com_ref, hg_ref, en_ref = cz.centroidal(m6, q[:, b], qd[:, b])
        ag_ref = cz.cmm(m6, q[:, b])
        com, hg, en = mb.centroidal(q[:, b], qd[:, b])
        com0, ag = mb.com(q[:, b]), mb.cmm_raw(q[:, b])
        assert com.shape == (3,) and hg.shape == (6,) and en.shape == (2,) and ag.shape == (6 * n,)
        errs = (_scaled(com, com_ref), _scaled(com0, com_ref), _scaled(hg, hg_ref), _scaled(en, en_ref),
                _scaled(ag, ag_ref))
        worst = max(worst, *errs)
        assert max(errs) <= 1e-9, (case, b, errs)
        assert np.array_equal(com, com0), (case, b)  # one sweep, the same sums
    print(f"{case} com / centroidal / cmm host f64 {worst:.3e}")


@pytest.mark.parametrize("case", ["fr3", "chain12", "chain30", "general7"])
def test_identities(ffi, case):
    """hg = A_G qd; T = 1/2 qd^T sym(H) qd with H of multibody_crba; A_G[0:3]^T (0, 0, g) = rnea(q, 0, 0)
    (dU/dq); U = g M com_z."""
    mb, _, _ = xr.setup(case)
    n, M = mb.n, mb.total_mass
    q, qd = xr.inputs(mb, 6, 72)[:2]
    z = np.zeros(n)
    worst = [0.0] * 4
    for b in range(q.shape[1]):
        com, hg, en = mb.centroidal(q[:, b], qd[:, b])
        A = mb.cmm(q[:, b])
        assert A.shape == (6, n)
        e0 = _scaled(A @ qd[:, b], hg)
        H = mb.crba(q[:, b])
        Hs = np.triu(H) + np.triu(H, 1).T  # the upper triangle is the ABI's; sym() of either triangle
        T = 0.5 * qd[:, b] @ Hs @ qd[:, b]
        e1 = abs(en[0] - T) / (1.0 + abs(T))
        grav = mb.rnea(q[:, b], z, z)
        e2 = _scaled(A[:3].T @ np.array([0.0, 0.0, G]), grav)
        U = G * M * com[2]
        e3 = abs(en[1] - U) / (1.0 + abs(U))
        worst = [max(a, e) for a, e in zip(worst, (e0, e1, e2, e3))]
        assert e0 <= 1e-12 and e1 <= 1e-12 and e2 <= 1e-9, (case, b, e0, e1, e2)
        assert en[1] == U or e3 <= 1e-15, (case, b, en[1], U)
    print(f"{case} identities: A_G qd {worst[0]:.3e} T {worst[1]:.3e} gravity {worst[2]:.3e} U {worst[3]:.3e}")


@pytest.mark.parametrize("case", ["fr3", "chain30", "tree9", "floating14"])
def test_kernels_compile_for_gfx950(ffi, case):
    """hipRTC needs no device: every form (com / centroidal / cmm, fp32 / fp64) builds for gfx950 and
    calls the new lane function."""
    mb, _, _ = xr.setup(case)
    for which, lane in enumerate(("com_lane", "centroidal_lane", "cmm_lane")):
        for f64 in (0, 1):
            assert mb.centroidal_jit_compile(which, f64, "gfx950") > 0, (case, which, f64)
            src = mb.centroidal_jit_source(which, f64)
            assert src and "rbamd::dev::" + lane in src and "centroidal_body.hip.hpp" in src, (case, which, f64)


def test_which_out_of_range_is_an_argument_error(ffi):
    lib, mb = ffi.lib(), ffi.Multibody.new()
    for which in (-1, 3):
        assert lib.multibody_centroidal_jit_source(mb.handle, which, 1, 1 << 20, None, 0) == -ARG
        assert ffi.last_error() == "which must be 0 com, 1 centroidal or 2 cmm"
        assert lib.multibody_centroidal_jit_compile(mb.handle, which, 1, 1 << 20, None) == -ARG
    assert lib.multibody_centroidal_jit_compile(mb.handle, 0, 1, 0, None) == -ARG
    assert ffi.last_error() == "batch must be positive"


def test_alias_refusals(ffi):
    lib, mb = ffi.lib(), ffi.Multibody.new()
    bufs = [(ctypes.c_double * 64)() for _ in range(5)]
    p = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    d = [ctypes.cast(b, ctypes.POINTER(ctypes.c_double)) for b in bufs]
    for t in ("f32", "f64"):
        com, cen, cmm = (getattr(lib, f"multibody_{k}_batch_{t}") for k in ("com", "centroidal", "cmm"))
        assert com(mb.handle, p[0], p[0], 1, 1, None) == ARG
        assert ffi.last_error() == "com: an output array is also an input"
        assert cmm(mb.handle, p[0], p[0], 1, 1, None) == ARG
        assert ffi.last_error() == "cmm: an output array is also an input"
        for out in range(2, 5):
            for inp in range(2):
                a = list(p)
                a[out] = p[inp]
                assert cen(mb.handle, *a, 1, 1, None) == ARG, (out, inp)
                assert ffi.last_error() == "centroidal: an output array is also an input"
        for o, o2 in ((3, 2), (4, 2), (4, 3)):
            a = list(p)
            a[o] = p[o2]
            assert cen(mb.handle, *a, 1, 1, None) == ARG, (o, o2)
            assert ffi.last_error() == "centroidal: two outputs are the same array"
    assert lib.multibody_com(mb.handle, d[0], d[0]) == ARG
    assert lib.multibody_cmm(mb.handle, d[0], d[0]) == ARG
    assert lib.multibody_centroidal(mb.handle, d[0], d[1], d[2], d[2], d[4]) == ARG
    assert ffi.last_error() == "centroidal: two outputs are the same array"
    assert lib.multibody_centroidal(mb.handle, d[0], d[1], d[2], d[3], d[1]) == ARG
    assert ffi.last_error() == "centroidal: an output array is also an input"


@pytest.mark.parametrize("case", ["tree9", "floating14"])
def test_single_configuration_form_refuses_trees(ffi, case):
    mb, _, _ = xr.setup(case)
    z = np.zeros(mb.n)
    for call in (lambda: mb.com(z), lambda: mb.centroidal(z, z), lambda: mb.cmm(z)):
        with pytest.raises(ffi.RigidBodyError, match="serial revolute"):
            call()
    dp = ctypes.POINTER(ctypes.c_double)
    out = np.zeros(6 * mb.n)
    assert ffi.lib().multibody_cmm(mb.handle, z.ctypes.data_as(dp), out.ctypes.data_as(dp)) == UNSUPPORTED
