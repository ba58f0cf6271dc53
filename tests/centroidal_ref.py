"""Reference for the whole-body entry points (com / centroidal / cmm): the definitions of
include/rigidbody_batch.h ("centre of mass, centroidal momentum, energy") evaluated with the 6x6
Featherstone model (oracle/featherstone6.Model6) without touching it:

    world poses   R_j = R_parent E_j,  pos_j = pos_parent + R_parent r_j      Model6.poses(q), root to leaf
    velocities    v_j = X_j v_parent + S_j qd_j                               Model6.xforms(q), Model6.S
    m_j, c_j, Ic_j read from the 6x6 link inertia I[j] = [[Ic + m C C^T, m C], [m C^T, m 1]], C = skew(c_j)

    x_j = pos_j + R_j c_j        xd_j = R_j (lin_j + ang_j x c_j)
    com = sum m_j x_j / M        l = sum m_j xd_j        k = sum R_j Ic_j ang_j + m_j (x_j - com) x xd_j
    T = 1/2 sum m_j |xd_j|^2 + ang_j . Ic_j ang_j        U = g M com_z
    A_G column k = hg at qd = e_k

Model6's frames are the URDF link frames and it orders spatial vectors [rot; lin]; hg is [lin; ang]:
the swap happens once, here (v[:3] is ang_j, v[3:] lin_j).  Outputs follow the ABI's
single-configuration layout: com [3], hg [6], energy [2], ag [6 n] (element row + 6 col).  Models and
input ranges: ext_wrench_ref.setup / inputs.  Shared by tests/test_centroidal_host.py and
tests/test_gpu_centroidal.py.
"""
import numpy as np

G = 9.81


def link_inertials(m6):
    """(m [n], c [n, 3], Ic [n, 3, 3]) read from Model6.I."""
    m, c, Ic = np.zeros(m6.n), np.zeros((m6.n, 3)), np.zeros((m6.n, 3, 3))
    for j, I in enumerate(m6.I):
        m[j] = I[3, 3]
        mC = I[:3, 3:]
        h = np.array([mC[2, 1], mC[0, 2], mC[1, 0]])
        if m[j] > 0:
            c[j] = h / m[j]
        C = np.array([[0.0, -c[j][2], c[j][1]], [c[j][2], 0.0, -c[j][0]], [-c[j][1], c[j][0], 0.0]])
        Ic[j] = I[:3, :3] - m[j] * C @ C.T
    return m, c, Ic


def total_mass(m6):
    return link_inertials(m6)[0].sum()


def _kin(m6, q):
    """What depends on q alone: (m, c, Ic, M, R, X, x, com)."""
    n = m6.n
    m, c, Ic = link_inertials(m6)
    M = m.sum()
    poses, X = m6.poses(q), m6.xforms(q)
    R, pos = [None] * n, [None] * n
    for j in range(n):
        par = m6.parent[j]
        Ej, rj = poses[j]
        if par < 0:
            R[j], pos[j] = Ej, rj
        else:
            R[j], pos[j] = R[par] @ Ej, pos[par] + R[par] @ rj
    x = [pos[j] + R[j] @ c[j] for j in range(n)]
    com = sum(m[j] * x[j] for j in range(n)) / M
    return m, c, Ic, M, R, X, x, com


def _momentum(m6, kin, qd):
    """(hg [6], T) at the velocities qd."""
    n = m6.n
    m, c, Ic, M, R, X, x, com = kin
    v = [None] * n
    for j in range(n):
        par = m6.parent[j]
        v[j] = X[j] @ (np.zeros(6) if par < 0 else v[par]) + m6.S[j] * qd[j]
    xd = [R[j] @ (v[j][3:] + np.cross(v[j][:3], c[j])) for j in range(n)]
    lin = sum(m[j] * xd[j] for j in range(n))
    ang = sum(R[j] @ (Ic[j] @ v[j][:3]) + m[j] * np.cross(x[j] - com, xd[j]) for j in range(n))
    T = 0.5 * sum(m[j] * xd[j] @ xd[j] + v[j][:3] @ Ic[j] @ v[j][:3] for j in range(n))
    return np.concatenate([lin, ang]), T


def centroidal(m6, q, qd):
    """(com [3], hg [6], energy [2]) of one configuration."""
    kin = _kin(m6, np.asarray(q, float))
    hg, T = _momentum(m6, kin, np.asarray(qd, float))
    M, com = kin[3], kin[7]
    return com, hg, np.array([T, G * M * com[2]])


def cmm(m6, q):
    """ag [6 n]: column k (elements 6 k .. 6 k + 5) is hg at qd = e_k."""
    kin = _kin(m6, np.asarray(q, float))
    return np.concatenate([_momentum(m6, kin, e)[0] for e in np.eye(m6.n)])


def centroidal_batch(m6, q, qd):
    """q, qd [n, B] -> (com [3, B], hg [6, B], energy [2, B])."""
    cols = [centroidal(m6, q[:, b], qd[:, b]) for b in range(q.shape[1])]
    return tuple(np.stack([c[k] for c in cols], axis=1) for k in range(3))


def cmm_batch(m6, q):
    """q [n, B] -> ag [6 n, B]."""
    return np.stack([cmm(m6, q[:, b]) for b in range(q.shape[1])], axis=1)
