"""The reverse-mode gradient of the fused rollout, CPU side: the single-configuration entry point
(multibody_rollout_vjp runs the GPU lane body compiled for the host, rollout_vjp_body.hip.hpp), its
hipRTC kernel compiled for gfx950 without a device, and the argument checks of the batched entry
points beyond the enumerated contract (test_abi_contract.py), which return before any device call.

Reference (rollout_vjp_ref.py): Richardson central differences of the fp64 oracle's own rollout
along a direction.  Tolerance |<g, d> - ref| <= 1e-7 (1 + |ref|) on the configurations whose
reference is self-consistent to 1e-8: all 20 for FR3 and the general-axis chain; the oracle alone
gives 16-17 of 20 on the 12-link chain, where at least 3 in 4 must qualify.
"""
import ctypes

import numpy as np
import pytest

import rollout_vjp_ref as ref
from test_deriv_host import _model

NCFG = 20
DT = ref.DT
OK, NULL, ARG, UNSUPPORTED = 0, 1, 2, 6


@pytest.fixture(scope="module")
def ffi():
    from rigidbody_amd import ffi

    return ffi


def _single(mb, c, b, gq=None, gqd=None):
    """multibody_rollout_vjp on configuration b of a case: (g_q0 [n], g_qd0 [n], g_tau [K, n])."""
    gq = c["gq"] if gq is None else gq
    gqd = c["gqd"] if gqd is None else gqd
    return mb.rollout_vjp(c["q"][:, b], c["qd"][:, b], c["tau"][:, :, b], DT, gq[:, :, b], gqd[:, :, b])


def _all(mb, c):
    """The single-configuration gradient of every configuration, stacked [n, B], [n, B], [K, n, B]."""
    g = [_single(mb, c, b) for b in range(c["q"].shape[1])]
    return (np.stack([x[0] for x in g], axis=1), np.stack([x[1] for x in g], axis=1),
            np.stack([x[2] for x in g], axis=2))


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("name", ["fr3", "chain12", "general7"])
def test_single_vs_directional_reference(ffi, oracle_mod, name, K):
    mb, om, _ = _model(ffi, oracle_mod, name)
    c = ref.make_case(om, mb.n, NCFG, K, 7300 + K)
    want, cons = ref.directional(om, c)
    good = cons <= 1e-8
    got = ref.pairing(_all(mb, c), (c["dq"], c["dqd"], c["dtau"]))
    err = np.abs(got - want) / (1 + np.abs(want))
    print(f"{name} K={K}: {int(good.sum())} of {NCFG} references within 1e-8 (worst {cons.max():.2e}); "
          f"worst error on them {err[good].max():.2e}, on all {err.max():.2e}")
    assert good.sum() >= (NCFG * 3 // 4 if name == "chain12" else NCFG)
    assert err[good].max() <= 1e-7


def test_full_gradient_smallest_shape(ffi, oracle_mod):
    """3 links, K = 2: each of the 12 gradient entries against its own coordinate direction -- the
    index conventions of g_tau[k] and gq[k]."""
    from oracle import urdf_model
    from rigidbody_amd import chains

    xml = chains.synthetic_chain_urdf(3)
    mb = ffi.Multibody.from_urdf_string(xml)
    om = oracle_mod.Model(urdf_model.model_raw_from_urdf(xml))
    n, K, B = 3, 2, 2
    c = ref.make_case(om, n, B, K, 99)
    g = _all(mb, c)
    flat = np.concatenate([g[0], g[1], g[2].reshape(K * n, B)])
    worst = 0.0
    for e in range(2 * n + K * n):
        d = np.zeros((2 * n + K * n, B))
        d[e] = 1.0
        want, cons = ref.directional(om, c, (d[:n], d[n:2 * n], d[2 * n:].reshape(K, n, B)))
        assert cons.max() <= 1e-8, (e, cons)
        err = np.abs(flat[e] - want) / (1 + np.abs(want))
        worst = max(worst, err.max())
    print(f"3 links K=2: worst entry error {worst:.2e}")
    assert worst <= 1e-7


def _scaled(a, b):
    return float((np.abs(np.asarray(a) - np.asarray(b)) / (1 + np.abs(b))).max())


def test_structure(ffi, oracle_mod):
    mb, om, _ = _model(ffi, oracle_mod, "fr3")
    n = mb.n
    # K = 1, gq = 0: g_tau[0] = dt sym(H)^-1 gqd[0]
    c = ref.make_case(om, n, 4, 1, 511)
    for b in range(4):
        g = _single(mb, c, b, gq=np.zeros_like(c["gq"]))
        inv = mb.fd_deriv(c["q"][:, b], c["qd"][:, b], c["tau"][0, :, b])[3]
        assert _scaled(g[2][0], DT * inv @ c["gqd"][0, :, b]) <= 1e-12
    # K = 3: the recursion assembled from the host fd_deriv matrices
    K = 3
    c = ref.make_case(om, n, 4, K, 512)
    for b in range(4):
        q, v = c["q"][:, b].copy(), c["qd"][:, b].copy()
        J = []
        for k in range(K):
            a, Dq, Dv, Dt = mb.fd_deriv(q, v, c["tau"][k, :, b])
            J.append((Dq, Dv, Dt))
            v = v + DT * a
            q = q + DT * v
        lq, lv, gt = np.zeros(n), np.zeros(n), np.zeros((K, n))
        for k in reversed(range(K)):
            lq = lq + c["gq"][k, :, b]
            vb = lv + c["gqd"][k, :, b] + DT * lq
            ab = DT * vb
            gt[k] = J[k][2].T @ ab
            lq = lq + J[k][0].T @ ab
            lv = vb + J[k][1].T @ ab
        g = _single(mb, c, b)
        assert max(_scaled(g[0], lq), _scaled(g[1], lv), _scaled(g[2], gt)) <= 1e-10
        # linear in the cotangents
        g2 = _single(mb, c, b, gq=2 * c["gq"], gqd=2 * c["gqd"])
        for x, y in zip(g, g2):
            assert np.all(np.abs(y - 2 * x) <= 1e-14 * np.abs(2 * x))


def test_kernel_compiles_without_device(ffi):
    from rigidbody_amd import chains

    for mb in (ffi.Multibody.new(), ffi.Multibody.from_urdf_string(chains.synthetic_chain_urdf(12))):
        for f64 in (False, True):
            assert mb.rollout_vjp_jit_compile(f64) > 1000
        assert "rollout_vjp_lane<" in mb.rollout_vjp_jit_source(True)
    lib = ffi.lib()
    tree = ffi.Multibody.from_urdf_string(chains.tree_urdf(), ffi.URDF_TREE | ffi.GENERAL_AXES)
    c30 = ffi.Multibody.from_urdf_string(chains.synthetic_chain_urdf(30))
    buf = ctypes.create_string_buffer(b"x" * 15, 16)
    for m, needle in ((tree, "serial revolute"), (c30, "mass-matrix")):
        for f64 in (0, 1):
            assert lib.multibody_rollout_vjp_jit_compile(m.handle, f64, 1 << 20, b"gfx950") == -UNSUPPORTED
            assert needle in ffi.last_error()
            buf.raw = b"x" * 16
            assert lib.multibody_rollout_vjp_jit_source(m.handle, f64, 1 << 20, buf, 16) == 0
            assert buf.raw[0] == 0
        assert m.rollout_vjp_jit_source() == ""
    assert lib.multibody_rollout_vjp_jit_compile(None, 0, 1, None) == -NULL
    assert lib.multibody_rollout_vjp_jit_compile(tree.handle, 0, 0, None) == -ARG
    assert ffi.last_error() == "batch must be positive"


def test_argument_checks(ffi):
    """K == 0, aliased arrays, models out of scope: refused before any device call (the pointers are
    never dereferenced); an empty batch has nothing to do whatever the model."""
    from rigidbody_amd import chains

    lib = ffi.lib()
    mb = ffi.Multibody.new()
    tree = ffi.Multibody.from_urdf_string(chains.tree_urdf(), ffi.URDF_TREE | ffi.GENERAL_AXES)
    c30 = ffi.Multibody.from_urdf_string(chains.synthetic_chain_urdf(30))
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(9)]  # q qd tau_seq gq gqd | g_q0 g_qd0 g_tau work

    def dev(fn, h, a, K=1, batch=8):
        return fn(h, a[0], a[1], a[2], 0.01, K, *a[3:9], batch, batch, None)

    def host(fn, h, a, K=1, batch=8):
        return fn(h, a[0], a[1], a[2], 0.01, K, *a[3:8], batch)

    for t in ("f32", "f64"):
        for call, fn, nptr in ((dev, getattr(lib, f"multibody_rollout_vjp_batch_{t}"), 9),
                               (host, getattr(lib, f"multibody_rollout_vjp_batch_host_{t}"), 8)):
            assert call(fn, mb.handle, p, K=0) == ARG and "K == 0" in ffi.last_error()
            assert call(fn, mb.handle, p, K=-2) == ARG and ffi.last_error() == "negative step count"
            assert call(fn, mb.handle, [None] * 9, K=0) == ARG  # the step count before the arrays
            assert call(fn, mb.handle, p, K=0, batch=0) == OK   # ... the empty batch before both
            for o in range(5, nptr):
                for i in range(5):
                    a = list(p)
                    a[o] = p[i]
                    assert call(fn, mb.handle, a) == ARG, (o, i)
                    assert ffi.last_error() == "rollout_vjp: an output array is also an input"
                for o2 in range(5, o):
                    a = list(p)
                    a[o] = p[o2]
                    assert call(fn, mb.handle, a) == ARG, (o, o2)
                    assert ffi.last_error() == "rollout_vjp: two outputs are the same array"
            for m, needle in ((tree, "serial revolute"), (c30, "mass-matrix")):
                assert call(fn, m.handle, p, batch=1) == UNSUPPORTED
                assert needle in ffi.last_error()
                assert call(fn, m.handle, p, batch=0) == OK
    z = (ctypes.c_double * 64)()
    w = [(ctypes.c_double * 64)() for _ in range(3)]
    one = lib.multibody_rollout_vjp
    assert one(None, z, z, z, 0.01, 1, z, z, *w) == NULL
    assert one(mb.handle, z, z, z, 0.01, 0, z, z, *w) == ARG and "K == 0" in ffi.last_error()
    assert one(mb.handle, z, z, z, 0.01, -1, z, z, *w) == ARG
    assert one(mb.handle, z, z, None, 0.01, 1, z, z, *w) == NULL and ffi.last_error() == "NULL array"
    assert one(mb.handle, z, z, z, 0.01, 1, z, z, w[0], w[1], None) == NULL
    assert one(mb.handle, z, z, z, 0.01, 1, z, z, w[0], z, w[2]) == ARG
    assert one(mb.handle, z, z, z, 0.01, 1, z, z, w[0], w[0], w[2]) == ARG
    assert one(tree.handle, z, z, z, 0.01, 1, z, z, *w) == UNSUPPORTED
    assert one(c30.handle, z, z, z, 0.01, 1, z, z, *w) == UNSUPPORTED and "mass-matrix" in ffi.last_error()
    assert one(mb.handle, z, z, z, 0.01, 1, z, z, *w) == OK
    with pytest.raises(ValueError):
        mb.rollout_vjp(np.zeros(7), np.zeros(7), np.zeros((2, 7)), 0.01, np.zeros((2, 7)), np.zeros((3, 7)))
