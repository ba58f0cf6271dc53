"""External link wrenches without a GPU: the single-configuration host forms multibody_rnea_ext /
multibody_fd_ext (the kernels' lane bodies compiled for the host, ext_body.hip.hpp), the hipRTC
compile of every kernel form, and the argument checks the new entry points add.  Reference:
tests/ext_wrench_ref.py (the fp64 oracle plus J^T f composed from the 6x6 model's transforms);
bounds are the header's fp64 contracts."""
import ctypes

import numpy as np
import pytest

import ext_wrench_ref as xr

ARG, UNSUPPORTED = 2, 6  # rb_status


@pytest.fixture(scope="module")
def ffi():
    from rigidbody_amd import ffi

    if not hasattr(ffi.Multibody, "rnea_ext"):
        pytest.fail("the binding has no external-wrench entry points")
    return ffi


def _scaled(got, ref, extra=0.0):
    return (np.abs(np.asarray(got) - ref) / (1.0 + np.abs(ref) + extra)).max()


@pytest.mark.parametrize("case", ["fr3", "chain12"])
def test_single_configuration_against_reference(ffi, case):
    mb, om, m6 = xr.setup(case)
    q, qd, qdd, tau, fext = xr.inputs(mb, 20, 31)
    for b in range(20):
        jtf = xr.jt_f(m6, q[:, b], fext[:, b])
        ref = om.rnea(q[:, b], qd[:, b], qdd[:, b]) - jtf
        got = mb.rnea_ext(q[:, b], qd[:, b], qdd[:, b], fext[:, b])
        assert _scaled(got, ref) <= 1e-9, (case, b)
        acc = mb.fd_ext(q[:, b], qd[:, b], tau[:, b], fext[:, b])
        back = mb.rnea_ext(q[:, b], qd[:, b], acc, fext[:, b])
        assert _scaled(back, tau[:, b], np.abs(jtf)) <= 1e-8, (case, b)


def test_last_link_wrench_is_jacobian_transpose(ffi):
    mb, _, _ = xr.setup("fr3")
    n = mb.n
    q, qd, qdd, _, fext = xr.inputs(mb, 20, 32)
    fext[: 6 * (n - 1)] = 0.0
    for b in range(20):
        f = fext[6 * (n - 1):, b]
        J = mb.jac_raw(q[:, b]).reshape(n, 6)  # column j of the 6 x n Jacobian, rows [lin; rot]
        d = mb.rnea(q[:, b], qd[:, b], qdd[:, b]) - mb.rnea_ext(q[:, b], qd[:, b], qdd[:, b], fext[:, b])
        assert _scaled(d, J @ f) <= 1e-9, b


def test_wrench_reaches_only_ancestors(ffi):
    """A wrench on link 2 of the serial chain leaves every tau_i, i > 2, bit-equal to the plain
    RNEA's (those links are no ancestors of link 2), and moves the others."""
    mb, _, _ = xr.setup("fr3")
    q, qd, qdd, _, fext = xr.inputs(mb, 20, 33)
    fext[:12] = 0.0
    fext[18:] = 0.0
    for b in range(20):
        plain = mb.rnea(q[:, b], qd[:, b], qdd[:, b])
        got = mb.rnea_ext(q[:, b], qd[:, b], qdd[:, b], fext[:, b])
        assert np.array_equal(got[3:], plain[3:]), b
        assert np.all(got[2] != plain[2]), b


CASES = ["fr3", "general12", "chain30", "tree9", "floating14"]


@pytest.mark.parametrize("case", CASES)
def test_kernels_compile_for_gfx950(ffi, case):
    """hipRTC needs no device: every form (rnea_ext / fd_ext, fp32 / fp64) builds for gfx950 and
    calls the new lane function."""
    mb, _, _ = xr.setup(case)
    for fd, lane in ((0, "rnea_ext_lane"), (1, "fd_ext_lane")):
        for f64 in (0, 1):
            assert mb.ext_jit_compile(fd, f64, "gfx950") > 0, (case, fd, f64)
            src = mb.ext_jit_source(fd, f64)
            assert "rbamd::dev::" + lane in src and "kExtRa" in src, (case, fd, f64)
    form = "true" if case in ("fr3", "general12") else "false"  # mass-matrix FD up to 12 serial links
    assert f"Topo, {form}>" in mb.ext_jit_source(1, 1)


def test_alias_refusals(ffi):
    lib, mb = ffi.lib(), ffi.Multibody.new()
    bufs = [(ctypes.c_double * 64)() for _ in range(5)]
    p = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    for op in ("rnea_ext", "fd_ext"):
        for i in range(4):
            args = p[:4] + [p[i]]  # the output is input i
            for t in ("f32", "f64"):
                assert getattr(lib, f"multibody_{op}_batch_{t}")(mb.handle, *args, 1, 1, None) == ARG, (op, i, t)
                assert ffi.last_error() == f"{op}: an output array is also an input (no in-place form)"
            d = [ctypes.cast(b, ctypes.POINTER(ctypes.c_double)) for b in bufs[:4]]
            assert getattr(lib, f"multibody_{op}")(mb.handle, *d, d[i]) == ARG, (op, i)
            assert ffi.last_error().startswith(op + ":")


def test_single_configuration_form_refuses_trees(ffi):
    mb, _, _ = xr.setup("tree9")
    z = np.zeros(mb.n)
    for call in (mb.rnea_ext, mb.fd_ext):
        with pytest.raises(ffi.RigidBodyError, match="serial revolute"):
            call(z, z, z, np.zeros(6 * mb.n))
    d = z.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    f = np.zeros(6 * mb.n).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = np.zeros(mb.n).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert ffi.lib().multibody_rnea_ext(mb.handle, d, d, d, f, out) == UNSUPPORTED
