"""Reference for the external-wrench entry points (rnea_ext / fd_ext), composed from the fp64
oracle -- which has no external forces -- and the 6x6 Featherstone model's own transforms:

    tau_ref = om.rnea_batch(q, qd, qdd) - J^T f        qdd_ref = om.fd_batch(q, qd, tau + J^T f)

with (J^T f)_j = S_j^T F_j and F_j = fext_j + sum_children X_c^T F_c propagated leaf to root.
Model6 orders spatial vectors [rot; lin], the ABI's fext rows are [lin; rot] per link (force, then
moment): the swap happens once, in jt_f.  Shared by tests/test_ext_host.py and tests/test_gpu_ext.py.
"""
import numpy as np

FORCE, MOMENT = 20.0, 5.0  # N, N m: wrench components are uniform in +- these


def jt_f(m6, q, fext):
    """sum_j J_j(q)^T fext_j of one configuration: q [n], fext [6 n] (ABI order) -> [n]."""
    n = m6.n
    f = np.asarray(fext, float).reshape(n, 6)
    F = [np.concatenate([f[j, 3:], f[j, :3]]) for j in range(n)]
    X = m6.xforms(np.asarray(q, float))
    out = np.zeros(n)
    for j in range(n - 1, -1, -1):
        out[j] = m6.S[j] @ F[j]
        p = m6.parent[j]
        if p >= 0:
            F[p] = F[p] + X[j].T @ F[j]
    return out


def jt_f_batch(m6, q, fext):
    """q [n, B], fext [6 n, B] -> [n, B]."""
    return np.stack([jt_f(m6, q[:, b], fext[:, b]) for b in range(q.shape[1])], axis=1)


def setup(case):
    """(Multibody, oracle.Model, Model6) of a named model: fr3, chainN (the reference's reading of the
    synthetic z-axis chain), generalN (serial chain with general axes), tree9, floating14."""
    from oracle import featherstone6, oracle, urdf_model
    from rigidbody_amd import chains, ffi

    if case == "fr3" or case.startswith("chain"):
        xml = chains.fr3_urdf_text() if case == "fr3" else chains.synthetic_chain_urdf(int(case[5:]))
        raw = urdf_model.model_raw_from_urdf(xml)
        return ffi.Multibody.from_urdf_string(xml), oracle.Model(raw), featherstone6.Model6(raw)
    if case.startswith("general"):
        xml, flags, floating = chains.general_chain_urdf(int(case[7:])), ffi.URDF_TREE | ffi.GENERAL_AXES, False
    else:
        floating = case.startswith("floating")
        xml = chains.tree_urdf(floating=floating)
        flags = ffi.FLOATING_BASE if floating else ffi.URDF_TREE | ffi.GENERAL_AXES
    fr = urdf_model.model_frames_from_urdf_tree(xml, floating=floating)
    return (ffi.Multibody.from_urdf_string(xml, flags), oracle.Model(frames=fr, general=True),
            featherstone6.Model6(frames=fr, general=True))


def inputs(mb, B, seed):
    """q, qd, qdd, tau [n, B] over chains.input_ranges (as tests/test_gpu_tree.py) and fext [6 n, B]."""
    from rigidbody_amd import chains

    lim = mb.limits()
    rng = np.random.default_rng(seed)
    out = []
    for kind in ("q", "qd", "qdd", "tau"):
        lo, hi = (np.asarray(x, float) for x in chains.input_ranges(lim, kind))
        out.append(lo[:, None] + (hi - lo)[:, None] * rng.random((mb.n, B)))
    amp = np.tile([FORCE] * 3 + [MOMENT] * 3, mb.n)[:, None]
    out.append(amp * (2.0 * rng.random((6 * mb.n, B)) - 1.0))
    return out
