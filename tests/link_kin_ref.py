"""Reference for the link-kinematics entry points (link_pose / link_vel), built on the 6x6 Featherstone
model (oracle/featherstone6.Model6) without touching it:

    world poses   R_j = R_parent E_j,  p_j = p_parent + R_parent r_j   from Model6.poses(q), root to leaf
    velocities    v_j = X_j v_parent + S_j qd_j                        from Model6.xforms(q) and Model6.S

Model6's frames are the URDF link frames themselves (it never changes a link's axes) and it orders
spatial vectors [rot; lin]; the ABI's vel rows are [lin; rot] per link: the swap happens once, here.
Outputs follow the ABI's single-configuration layout: pos [3 n], rot [9 n] (link j's R_j column-major,
element row + 3 col), vel [6 n].  Models and input ranges: ext_wrench_ref.setup / inputs.  Shared by
tests/test_link_kin_host.py and tests/test_gpu_link_kin.py.
"""
import numpy as np


def link_kin(m6, q, qd):
    """(pos [3 n], rot [9 n], vel [6 n]) of one configuration."""
    n = m6.n
    q, qd = np.asarray(q, float), np.asarray(qd, float)
    poses, X = m6.poses(q), m6.xforms(q)
    R, p, v = [None] * n, [None] * n, [None] * n
    for j in range(n):
        par = m6.parent[j]
        Ej, rj = poses[j]
        if par < 0:
            R[j], p[j] = Ej, rj
        else:
            R[j], p[j] = R[par] @ Ej, p[par] + R[par] @ rj
        v[j] = X[j] @ (np.zeros(6) if par < 0 else v[par]) + m6.S[j] * qd[j]
    pos = np.concatenate(p)
    rot = np.concatenate([Rj.T.reshape(-1) for Rj in R])  # column-major: element (row, col) at row + 3 col
    vel = np.concatenate([np.concatenate([vj[3:], vj[:3]]) for vj in v])
    return pos, rot, vel


def link_kin_batch(m6, q, qd):
    """q, qd [n, B] -> (pos [3 n, B], rot [9 n, B], vel [6 n, B])."""
    cols = [link_kin(m6, q[:, b], qd[:, b]) for b in range(q.shape[1])]
    return tuple(np.stack([c[k] for c in cols], axis=1) for k in range(3))
