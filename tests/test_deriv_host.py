"""Analytical derivatives of the inverse and forward dynamics, CPU side: the single-configuration
entry points (multibody_rnea_deriv / multibody_fd_deriv run the GPU lane body compiled for the
host, rnea_deriv_body.hip.hpp), the hipRTC kinds 7 / 8 compiled for gfx950 without a device, and
the argument checks of the batched entry points, which return before any device call.

Reference (deriv_ref.py): Richardson-extrapolated central differences of the fp64 oracle, whose
own consistency (extrapolations from two step pairs) every test asserts first at 1e-9 scaled;
measured 3e-11 (FR3), 2e-10 (12 links), 1e-11 (general axes) on these inputs.  Tolerances:
rnea derivatives 1e-8 (1 + |ref|), 100x that; forward-dynamics derivatives against differences of
the oracle's fd 1e-6 (1 + |ref|) on the configurations where that reference is self-consistent to
1e-7 (the solve amplifies its rounding by cond(H) |qdd| / h: all 20 FR3 configurations qualify,
about 3 in 4 of the 12-link chain's), and on every configuration, exactly, through their defining
identities with sym(H) from crba, at 1e-9 / 1e-8 (measured 1e-13).
"""
import ctypes

import numpy as np
import pytest

import deriv_ref
from conftest import load_json

NCFG = 20


@pytest.fixture(scope="module")
def ffi():
    from rigidbody_amd import ffi

    return ffi


def _model(ffi, oracle_mod, name):
    """(Multibody, oracle model, per-kind (lo, hi))."""
    from oracle import urdf_model
    from rigidbody_amd import chains

    if name == "general7":
        xml = chains.general_chain_urdf(7)
        mb = ffi.Multibody.from_urdf_string(xml, ffi.GENERAL_AXES | ffi.URDF_TREE)
        om = oracle_mod.Model(frames=urdf_model.model_frames_from_urdf_tree(xml), general=True)
        rng = {"q": 2.5, "qd": 2.0, "qdd": 5.0, "tau": 5.0}
        return mb, om, {k: ([-v] * 7, [v] * 7) for k, v in rng.items()}
    xml = chains.fr3_urdf_text() if name == "fr3" else chains.synthetic_chain_urdf(12)
    mb = ffi.Multibody.from_urdf_string(xml)
    om = oracle_mod.Model(urdf_model.model_raw_from_urdf(xml))
    return mb, om, {k: chains.input_ranges(mb.limits(), k) for k in ("q", "qd", "qdd", "tau")}


def _inputs(mb, ranges, kinds, B, seed):
    from rigidbody_amd import chains

    return [chains.host_uniform(mb.n, B, *ranges[k], seed + i) for i, k in enumerate(kinds)]


@pytest.mark.parametrize("name", ["fr3", "chain12", "general7"])
def test_rnea_deriv_single_vs_reference(ffi, oracle_mod, name):
    mb, om, ranges = _model(ffi, oracle_mod, name)
    q, qd, qdd = _inputs(mb, ranges, ("q", "qd", "qdd"), NCFG, 4100)
    if name == "fr3":
        g = load_json("main_cpp_case.json")["cases"]["main_cpp"]
        q, qd, qdd = (np.column_stack([a, np.asarray(g[k], float)]) for a, k in ((q, "q"), (qd, "dq"), (qdd, "ddq")))
    rq, rqd, cons = deriv_ref.rnea_deriv_ref(om, q, qd, qdd)
    print(f"{name}: reference consistency {cons.max():.2e}")
    assert cons.max() <= 1e-9
    n = mb.n
    worst = 0.0
    for b in range(q.shape[1]):
        dq, dqd = mb.rnea_deriv(q[:, b], qd[:, b], qdd[:, b])
        worst = max(worst, deriv_ref.scaled(dq, rq[:, b].reshape(n, n).T), deriv_ref.scaled(dqd, rqd[:, b].reshape(n, n).T))
    print(f"{name}: max scaled error {worst:.2e}")
    assert worst <= 1e-8


def test_rnea_deriv_structure(ffi, oracle_mod):
    """dtau_dqd vanishes at qd = 0 (rnea is quadratic in qd); d tau / d qdd, by differences of the
    host rnea (affine in qdd, so exact), is sym(H) of crba; each output can be left out."""
    mb, om, ranges = _model(ffi, oracle_mod, "fr3")
    q, qdd = _inputs(mb, ranges, ("q", "qdd"), 1, 77)
    q, qdd, n = q[:, 0], qdd[:, 0], mb.n
    dq, dqd = mb.rnea_deriv(q, np.zeros(n), qdd)
    assert np.abs(dqd).max() <= 1e-13 * (1 + np.abs(dq).max())
    qd = np.linspace(-1, 1, n)
    H = mb.crba(q)
    H = np.triu(H) + np.triu(H, 1).T
    base = mb.rnea(q, qd, qdd)
    dqdd = np.column_stack([mb.rnea(q, qd, qdd + np.eye(n)[k]) - base for k in range(n)])
    assert np.abs(dqdd - H).max() <= 1e-12 * (1 + np.abs(base).max())
    lib = ffi.lib()
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    full = mb.rnea_deriv(q, qd, qdd)
    only = np.full(n * n, 7.0)
    assert lib.multibody_rnea_deriv(mb.handle, p(q), p(qd), p(qdd), p(only), None) == 0
    assert np.array_equal(only.reshape(n, n).T, full[0])
    assert lib.multibody_rnea_deriv(mb.handle, p(q), p(qd), p(qdd), None, p(only)) == 0
    assert np.array_equal(only.reshape(n, n).T, full[1])


@pytest.mark.parametrize("name", ["fr3", "chain12"])
def test_fd_deriv_single(ffi, oracle_mod, name):
    mb, om, ranges = _model(ffi, oracle_mod, name)
    q, qd, tau = _inputs(mb, ranges, ("q", "qd", "tau"), NCFG, 5200)
    rq, rqd, cons = deriv_ref.fd_deriv_ref(om, q, qd, tau)
    qdd_ref = om.fd_batch(q, qd, tau)
    Hs = deriv_ref.sym_h(om, q)
    # differences of a solve carry its rounding, eps cond(H) |qdd| / h, so this reference is judged
    # per configuration: one that is not self-consistent to a tenth of the 1e-6 tolerance is not
    # compared against (its identities below still are); most must qualify
    good = cons <= 1e-7
    print(f"{name}: fd reference consistency median {np.median(cons):.2e} max {cons.max():.2e}, "
          f"{int(good.sum())} of {NCFG} within 1e-7, cond(H) up to {max(np.linalg.cond(h) for h in Hs):.1e}")
    assert good.sum() >= NCFG // 2
    n = mb.n
    w = dict(qdd=0.0, qdd_oracle=0.0, inv=0.0, idq=0.0, idqd=0.0, fdq=0.0, fdqd=0.0)
    for b in range(NCFG):
        qdd, fq, fqd, ft = mb.fd_deriv(q[:, b], qd[:, b], tau[:, b])
        # the host forward dynamics: the definition, residual through the host rnea
        w["qdd"] = max(w["qdd"], deriv_ref.scaled(mb.rnea(q[:, b], qd[:, b], qdd), tau[:, b]))
        w["qdd_oracle"] = max(w["qdd_oracle"], deriv_ref.scaled(qdd, qdd_ref[:, b]))
        H = mb.crba(q[:, b])
        H = np.triu(H) + np.triu(H, 1).T
        w["inv"] = max(w["inv"], deriv_ref.scaled(H @ ft, np.eye(n)))
        assert np.array_equal(ft, ft.T) or deriv_ref.scaled(ft, ft.T) <= 1e-12
        dq, dqd = mb.rnea_deriv(q[:, b], qd[:, b], qdd)
        w["idq"] = max(w["idq"], deriv_ref.scaled(H @ fq, -dq))
        w["idqd"] = max(w["idqd"], deriv_ref.scaled(H @ fqd, -dqd))
        if good[b]:
            w["fdq"] = max(w["fdq"], deriv_ref.scaled(fq, rq[:, b].reshape(n, n).T))
            w["fdqd"] = max(w["fdqd"], deriv_ref.scaled(fqd, rqd[:, b].reshape(n, n).T))
    print(name, {k: f"{v:.2e}" for k, v in w.items()})
    # qdd: the definition's torque residual through the host rnea, and the oracle's solve (header:
    # |qdd - exact| <= 4 eps64 cond(H) (1 + |qdd|), cond <= 2e4 here: 2e-11)
    assert w["qdd"] <= 1e-9 and w["qdd_oracle"] <= 1e-9
    assert w["inv"] <= 1e-9
    assert w["idq"] <= 1e-8 and w["idqd"] <= 1e-8
    assert w["fdq"] <= 1e-6 and w["fdqd"] <= 1e-6


def test_jit_kinds_compile_without_device(ffi):
    from rigidbody_amd import chains

    mb = ffi.Multibody.new()
    for kind, lane in (("rnea_deriv", "rnea_deriv_lane"), ("fd_deriv", "fd_deriv_lane")):
        for f64 in (False, True):
            assert mb.jit_compile(kind=kind, f64=f64, arch="gfx950") > 1000
        assert lane in mb.jit_source(kind=kind, f64=True)
    tree = ffi.Multibody.from_urdf_string(chains.tree_urdf(), ffi.URDF_TREE | ffi.GENERAL_AXES)
    c30 = ffi.Multibody.from_urdf_string(chains.synthetic_chain_urdf(30))
    lib = ffi.lib()
    for m, kinds in ((tree, (7, 8)), (c30, (8,))):
        for k in kinds:
            assert lib.multibody_jit_compile_ex(m.handle, k, 1, 1 << 20, 0, b"gfx950") == -6  # RB_ERR_UNSUPPORTED
            assert "no such kernel for this model" in ffi.last_error()
            assert lib.multibody_jit_source_ex(m.handle, k, 1, 1 << 20, 0, None, 0) == 0  # the empty source
            assert lib.multibody_kernel_form_ex(m.handle, k, 1, 1 << 20, 0) == -6
    assert "mass-matrix" in ffi.last_error()
    assert "rnea_deriv_lane" in c30.jit_source(kind="rnea_deriv")
    with pytest.raises(ffi.RigidBodyError, match="serial revolute"):
        tree.rnea_deriv(np.zeros(tree.n), np.zeros(tree.n), np.zeros(tree.n))
    with pytest.raises(ffi.RigidBodyError, match="mass-matrix"):
        c30.fd_deriv(np.zeros(30), np.zeros(30), np.zeros(30))


def test_bad_arguments_refused_before_the_device(ffi):
    """NULL handle, every output NULL, ld < batch, an aliased output, an out-of-scope model: the
    documented status, before any device call (no GPU here; the pointers are never dereferenced)."""
    from rigidbody_amd import chains

    lib = ffi.lib()
    mb = ffi.Multibody.new()
    a, b, c, d, e, f, g = (ctypes.c_void_p(4096 * (i + 1)) for i in range(7))
    for t in ("f32", "f64"):
        rd = getattr(lib, f"multibody_rnea_deriv_batch_{t}")
        fd = getattr(lib, f"multibody_fd_deriv_batch_{t}")
        rh = getattr(lib, f"multibody_rnea_deriv_batch_host_{t}")
        fh = getattr(lib, f"multibody_fd_deriv_batch_host_{t}")
        assert rd(None, a, b, c, d, e, 8, 8, None) == 1 and "NULL" in ffi.last_error()
        assert fd(None, a, b, c, d, e, f, g, 8, 8, None) == 1
        assert rh(None, a, b, c, d, e, 8) == 1 and fh(None, a, b, c, d, e, f, g, 8) == 1
        assert rd(mb.handle, a, b, c, None, None, 8, 8, None) == 1 and "output" in ffi.last_error()
        assert fd(mb.handle, a, b, c, None, None, None, None, 8, 8, None) == 1
        assert rh(mb.handle, a, b, c, None, None, 8) == 1 and fh(mb.handle, a, b, c, None, None, None, None, 8) == 1
        assert rd(mb.handle, a, None, c, d, e, 8, 8, None) == 1
        assert rd(mb.handle, a, b, c, d, e, 8, 7, None) == 2 and "ld" in ffi.last_error()
        assert fd(mb.handle, a, b, c, d, e, f, g, 8, 7, None) == 2
        assert rd(mb.handle, a, b, c, d, e, -1, 8, None) == 2
        assert rd(mb.handle, a, b, c, c, e, 8, 8, None) == 2 and "input" in ffi.last_error()
        assert rd(mb.handle, a, b, c, d, d, 8, 8, None) == 2 and "same array" in ffi.last_error()
        assert fd(mb.handle, a, b, c, a, e, f, g, 8, 8, None) == 2
        assert fd(mb.handle, a, b, c, d, e, f, e, 8, 8, None) == 2
        assert fh(mb.handle, a, b, c, d, e, f, d, 8) == 2
        assert rd(mb.handle, a, b, c, d, e, 0, 0, None) == 0  # empty batch: nothing to do
    tree = ffi.Multibody.from_urdf_string(chains.tree_urdf(), ffi.URDF_TREE | ffi.GENERAL_AXES)
    c30 = ffi.Multibody.from_urdf_string(chains.synthetic_chain_urdf(30))
    assert lib.multibody_rnea_deriv_batch_f64(tree.handle, a, b, c, d, e, 8, 8, None) == 6
    assert lib.multibody_fd_deriv_batch_f64(tree.handle, a, b, c, d, e, f, g, 8, 8, None) == 6
    assert lib.multibody_fd_deriv_batch_f32(c30.handle, a, b, c, d, e, f, g, 8, 8, None) == 6
    assert "12 links" in ffi.last_error()
    assert lib.multibody_fd_deriv_batch_host_f64(c30.handle, a, b, c, d, e, f, g, 8) == 6
    p = ctypes.POINTER(ctypes.c_double)
    z = (ctypes.c_double * 64)()
    assert lib.multibody_rnea_deriv(None, z, z, z, z, z) == 1
    assert lib.multibody_rnea_deriv(mb.handle, z, z, z, ctypes.cast(None, p), ctypes.cast(None, p)) == 1
    assert lib.multibody_fd_deriv(mb.handle, z, z, None, z, z, z, z) == 1
    # the wrappers check shapes before the library reads n values from each vector
    with pytest.raises(ValueError):
        mb.rnea_deriv(np.zeros(6), np.zeros(7), np.zeros(7))
    with pytest.raises(ValueError, match=r"\[7, B\]"):
        mb.rnea_deriv_batch_host(np.zeros((7, 3)), np.zeros((7, 2)), np.zeros((7, 3)))
