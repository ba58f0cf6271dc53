"""The reverse-mode gradient of the fused contact rollout, CPU side: the single-configuration entry
point (multibody_rollout_contact_vjp runs the GPU lane body compiled for the host,
contact_vjp_body.hip.hpp), its hipRTC kernel compiled for gfx950 without a device, and the argument
checks of the batched entry points, which return before any device call.

Reference, inputs and the qualification rule: contact_vjp_ref.py (Richardson central differences of
a rollout assembled from the reference contact law and the fp64 oracle, 40 configurations, K = 3,
dt = 1e-3; at least 32 must be self-consistent to 1e-8, and on those
|<g, d> - ref| <= 1e-7 (1 + |ref|)).
"""
import ctypes

import numpy as np
import pytest

import contact_ref as cr
import contact_vjp_ref as ref

DT = ref.DT
OK, NULL, ARG, UNSUPPORTED = 0, 1, 2, 6
MODELS = ["fr3", "chain12", "general7"]


@pytest.fixture(scope="module")
def ffi():
    from rigidbody_amd import ffi

    return ffi


def _all(fn, c):
    """A single-configuration gradient on every configuration, stacked [n, B], [n, B], [K, n, B]."""
    g = [fn(c["q"][:, b], c["qd"][:, b], c["tau"][:, :, b], DT, c["gq"][:, :, b], c["gqd"][:, :, b])
         for b in range(c["q"].shape[1])]
    return (np.stack([x[0] for x in g], axis=1), np.stack([x[1] for x in g], axis=1),
            np.stack([x[2] for x in g], axis=2))


@pytest.mark.parametrize("name", MODELS)
def test_directional_against_reference(ffi, name):
    """Measured (host body, fp64): FR3 39 of 40 qualify, worst error on them 1.0e-10; 12 links 36 of 40,
    2.8e-10; general-axis 7 links 40 of 40, 2.6e-10."""
    cs = ref.case(name)
    assert 0.25 <= cs["share"] <= 0.75
    ref.check(_all(cs["mb"].rollout_contact_vjp, cs["c"]), cs, label=name)


@pytest.mark.parametrize("name", MODELS)
def test_frictionless_path(ffi, name):
    """friction = 0: the kernel's friction terms are folded away; the directional test still holds."""
    cs = ref.case(name, friction=0.0)
    assert 0.25 <= cs["share"] <= 0.75
    ref.check(_all(cs["mb"].rollout_contact_vjp, cs["c"]), cs, label=f"{name} frictionless")


@pytest.mark.parametrize("off", ["stiffness", "plane"])
@pytest.mark.parametrize("name", MODELS)
def test_no_contact_equals_plain_gradient(ffi, name, off):
    """stiffness = 0, or the plane 10 m below every point: multibody_rollout_vjp on the plain handle, to
    1e-12 (1 + |ref|) -- the two forward passes take different bias sweeps, the gradients the same
    column sweeps; an inactive point contributes exactly zero."""
    base = ref.case(name)
    c, cm = base["c"], base["cm"]
    if off == "stiffness":
        over = dict(stiffness=0.0)
    else:
        _, _, m6 = ref.model(name)
        nh = np.asarray(cm["normal"], float)
        low = min((cr.point_kin(m6, cm["links"], cm["points"], c["q"][:, b], c["qd"][:, b])[0] @ nh).min()
                  for b in range(c["q"].shape[1]))
        over = dict(offset=float(low) - 10.0)
    mb, _ = ref.contact_model(name, c["q"], c["qd"], **over)
    got = _all(mb.rollout_contact_vjp, c)
    want = _all(base["plain"].rollout_vjp, c)
    worst = max(float((np.abs(g - w) / (1 + np.abs(w))).max()) for g, w in zip(got, want))
    print(f"{name} {off}: worst scaled difference to the plain gradient {worst:.2e}")
    assert worst <= 1e-12


def test_kernel_compiles_without_device(ffi):
    cs = ref.case("fr3")
    mb = cs["mb"]
    for f64 in (False, True):
        assert mb.contact_vjp_jit_compile(f64, "gfx950") > 1000
    assert "rollout_contact_vjp_lane<" in mb.contact_vjp_jit_source(True)
    assert ref.case("general7")["mb"].contact_vjp_jit_compile(True) > 1000
    lib = ffi.lib()
    plain = cs["plain"]
    tree = cr.setup("tree9", 4, 1)[0]
    c16 = cr.setup("chain16", 4, 1)[0]
    buf = ctypes.create_string_buffer(b"x" * 15, 16)
    for m, needle in ((plain, "multibody_with_contacts"), (tree, "serial revolute"), (c16, "mass-matrix")):
        for f64 in (0, 1):
            assert lib.multibody_contact_vjp_jit_compile(m.handle, f64, 1 << 20, b"gfx950") == -UNSUPPORTED
            assert needle in ffi.last_error()
            buf.raw = b"x" * 16
            assert lib.multibody_contact_vjp_jit_source(m.handle, f64, 1 << 20, buf, 16) == 0
            assert buf.raw[0] == 0
        assert m.contact_vjp_jit_source() == ""
    assert lib.multibody_contact_vjp_jit_compile(None, 0, 1, None) == -NULL
    assert lib.multibody_contact_vjp_jit_compile(mb.handle, 0, 0, None) == -ARG
    assert ffi.last_error() == "batch must be positive"


def test_argument_checks(ffi):
    """Every status in the check order: NULL handle and arrays, ld < batch, K < 0, K == 0, the empty
    batch, an aliased output or workspace, a handle without a contact set, a tree, a chain of 16 links
    -- refused before any device call (the pointers are never dereferenced)."""
    lib = ffi.lib()
    cs = ref.case("fr3")
    mb, plain = cs["mb"], cs["plain"]
    tree = cr.setup("tree9", 4, 1)[0]
    c16 = cr.setup("chain16", 4, 1)[0]
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(9)]  # q qd tau_seq gq gqd | g_q0 g_qd0 g_tau work

    def dev(fn, h, a, K=1, batch=8, ld=None):
        return fn(h, a[0], a[1], a[2], DT, K, *a[3:9], batch, batch if ld is None else ld, None)

    def host(fn, h, a, K=1, batch=8, ld=None):
        return fn(h, a[0], a[1], a[2], DT, K, *a[3:8], batch)

    for t in ("f32", "f64"):
        for call, fn, nptr in ((dev, getattr(lib, f"multibody_rollout_contact_vjp_batch_{t}"), 9),
                               (host, getattr(lib, f"multibody_rollout_contact_vjp_batch_host_{t}"), 8)):
            assert call(fn, None, p) == NULL and ffi.last_error() == "NULL Multibody handle"
            assert call(fn, mb.handle, p, batch=-1) == ARG and ffi.last_error() == "negative batch"
            if call is dev:
                assert call(fn, mb.handle, p, ld=7) == ARG and "ld < batch" in ffi.last_error()
            assert call(fn, mb.handle, p, K=-2) == ARG and ffi.last_error() == "negative step count"
            assert call(fn, mb.handle, p, K=0) == ARG
            assert ffi.last_error() == "rollout_contact_vjp: K == 0 steps, nothing to differentiate"
            assert call(fn, mb.handle, [None] * 9, K=0) == ARG  # the step count before the arrays
            assert call(fn, mb.handle, p, K=0, batch=0) == OK   # ... the empty batch before both
            for i in range(nptr):
                a = list(p)
                a[i] = None
                assert call(fn, mb.handle, a) == NULL and ffi.last_error() == "NULL array", i
            for o in range(5, nptr):
                for i in range(5):
                    a = list(p)
                    a[o] = p[i]
                    assert call(fn, mb.handle, a) == ARG, (o, i)
                    assert ffi.last_error() == "rollout_contact_vjp: an output array is also an input"
                for o2 in range(5, o):
                    a = list(p)
                    a[o] = p[o2]
                    assert call(fn, mb.handle, a) == ARG, (o, o2)
                    assert ffi.last_error() == "rollout_contact_vjp: two outputs are the same array"
            # the aliasing check comes before the contact set, the contact set before the scope
            a = list(p)
            a[5] = p[0]
            assert call(fn, plain.handle, a) == ARG
            for m, needle in ((plain, "multibody_with_contacts"), (tree, "serial revolute"), (c16, "mass-matrix")):
                assert call(fn, m.handle, p, batch=1) == UNSUPPORTED
                assert needle in ffi.last_error()
                assert call(fn, m.handle, p, batch=0) == OK
    z = (ctypes.c_double * 64)()
    w = [(ctypes.c_double * 64)() for _ in range(3)]
    one = lib.multibody_rollout_contact_vjp
    assert one(None, z, z, z, DT, 1, z, z, *w) == NULL
    assert one(mb.handle, z, z, z, DT, 0, z, z, *w) == ARG and "K == 0" in ffi.last_error()
    assert one(mb.handle, z, z, z, DT, -1, z, z, *w) == ARG
    assert one(mb.handle, z, z, None, DT, 1, z, z, *w) == NULL and ffi.last_error() == "NULL array"
    assert one(mb.handle, z, z, z, DT, 1, z, z, w[0], w[1], None) == NULL
    assert one(mb.handle, z, z, z, DT, 1, z, z, w[0], z, w[2]) == ARG
    assert one(mb.handle, z, z, z, DT, 1, z, z, w[0], w[0], w[2]) == ARG
    assert one(plain.handle, z, z, z, DT, 1, z, z, *w) == UNSUPPORTED and "multibody_with_contacts" in ffi.last_error()
    assert one(tree.handle, z, z, z, DT, 1, z, z, *w) == UNSUPPORTED and "serial revolute" in ffi.last_error()
    assert one(c16.handle, z, z, z, DT, 1, z, z, *w) == UNSUPPORTED and "mass-matrix" in ffi.last_error()
    assert one(mb.handle, z, z, z, DT, 1, z, z, *w) == OK
    with pytest.raises(ValueError):
        mb.rollout_contact_vjp(np.zeros(7), np.zeros(7), np.zeros((2, 7)), DT, np.zeros((2, 7)), np.zeros((3, 7)))
