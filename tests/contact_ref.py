"""Reference for the compliant-contact entry points (contact_wrench / rollout_contact), numpy fp64:
the header's law evaluated on link_kin_ref.link_kin, and per rollout step the oracle's forward
dynamics under the wrench, om.fd_batch(q, qd, tau + J^T fext) (ext_wrench_ref.jt_f), then the
semi-implicit Euler update.

    x_p = pos_l + R_l c_p                    xd_p = R_l (lin_l + ang_l x c_p)
    phi = max(d - nhat . x_p, 0)             phid = -nhat . xd_p
    f_n = max(k phi (1 + c phid), 0)         v_t  = xd_p + phid nhat
    F_p = f_n nhat - mu f_n v_t / sqrt(v_t . v_t + v_s^2)
    fext_l += [R_l^T F_p ; c_p x R_l^T F_p]

Point sets (points_for): a serial chain carries two points on its last link (multiplicity) and one
on a mid-chain link; a tree one on the leaf of every branch, a second one on the last leaf, and one
on the first link with more than one child (the torso: a branch link).  Points lie within 0.15 m of their
link's origin along each axis, except the set's first point, up to AMP = 0.8 m away: the clipped
branch of the normal force needs a separation speed above 1 / c = 2 m/s, which the models' joint speed
limits (a few rad/s) give a point only over a lever arm of that order (with every point within 0.15 m
no FR3, general5 or tree9 configuration out of 257 reaches it; with every point at 0.8 m the 30-link
chain clips so many that its active share leaves the band).
The plane's offset is the
median of nhat . x_p over all points and configurations of the test's initial batch, so about half
of the (point, configuration) pairs penetrate; every user asserts the reference's own active share
with check_share.  Shared by tests/test_contact_host.py and tests/test_gpu_contact.py.
"""
import numpy as np

import ext_wrench_ref as xr
import link_kin_ref as lk

NORMAL = (0.0, 0.0, 1.0)
PARAMS = dict(stiffness=2000.0, damping=0.5, friction=0.7, slip_velocity=0.01)
DT = 1e-3
AMP = 0.8


def points_for(mb):
    """(links, points [P, 3]) of the model's test contact set."""
    par, _ = mb.topology()
    n = mb.n
    kids = [[j for j in range(n) if par[j] == i] for i in range(n)]
    if all(par[j] == j - 1 for j in range(n)):
        links = [n - 1, n - 1, n // 2]
    else:
        leaves = [j for j in range(n) if not kids[j]]
        torso = next(j for j in range(n) if len(kids[j]) > 1)
        links = leaves + [leaves[-1], torso]
    rng = np.random.default_rng(1234 + n)
    points = rng.uniform(-0.15, 0.15, (len(links), 3))
    points[0] = rng.uniform(-AMP, AMP, 3)
    return links, points


def point_kin(m6, links, points, q, qd):
    """(x [P, 3], xd [P, 3], R [P, 3, 3]) of one configuration, base frame."""
    pos, rot, vel = lk.link_kin(m6, q, qd)
    x, xd, Rs = [], [], []
    for l, c in zip(links, points):
        R = rot[9 * l:9 * l + 9].reshape(3, 3).T  # column-major rows
        lin, ang = vel[6 * l:6 * l + 3], vel[6 * l + 3:6 * l + 6]
        x.append(pos[3 * l:3 * l + 3] + R @ c)
        xd.append(R @ (lin + np.cross(ang, c)))
        Rs.append(R)
    return np.array(x), np.array(xd), np.array(Rs)


def median_offset(m6, links, points, q, qd, normal=NORMAL):
    nh = np.asarray(normal, float)
    h = [point_kin(m6, links, points, q[:, b], qd[:, b])[0] @ nh for b in range(q.shape[1])]
    return float(np.median(np.concatenate(h)))


def contact(m6, cm, q, qd):
    """One configuration -> fext [6 n], cforce [3 P], info [P, 2] = (f_n, 1 + c phid) per point."""
    nh = np.asarray(cm["normal"], float)
    k, c, mu, vs = cm["stiffness"], cm["damping"], cm["friction"], cm["slip_velocity"]
    x, xd, Rs = point_kin(m6, cm["links"], cm["points"], q, qd)
    fext = np.zeros((m6.n, 6))
    cforce, info = [], []
    for p, l in enumerate(cm["links"]):
        phi = max(cm["offset"] - nh @ x[p], 0.0)
        phid = -(nh @ xd[p])
        fn = max(k * phi * (1.0 + c * phid), 0.0)
        vt = xd[p] + phid * nh
        F = fn * nh - mu * fn * vt / np.sqrt(vt @ vt + vs * vs)
        g = Rs[p].T @ F
        fext[l, :3] += g
        fext[l, 3:] += np.cross(cm["points"][p], g)
        cforce.append(F)
        info.append((fn, (1.0 + c * phid) if phi > 0 else np.nan))
    return fext.reshape(-1), np.concatenate(cforce), np.array(info)


def contact_batch(m6, cm, q, qd):
    """q, qd [n, B] -> fext [6 n, B], cforce [3 P, B], info [P, 2, B]."""
    cols = [contact(m6, cm, q[:, b], qd[:, b]) for b in range(q.shape[1])]
    return tuple(np.stack([col[i] for col in cols], axis=-1) for i in range(3))


def rollout(om, m6, cm, q, qd, tau_seq, dt=DT):
    """q, qd [n, B], tau_seq [K, n, B] -> traj [K, n, B], q_K, qd_K, info [K, P, 2, B]."""
    q, qd = np.array(q, float), np.array(qd, float)
    traj, infos = [], []
    for tau in tau_seq:
        fext, _, info = contact_batch(m6, cm, q, qd)
        a = om.fd_batch(q, qd, tau + xr.jt_f_batch(m6, q, fext))
        qd = qd + dt * a
        q = q + dt * qd
        traj.append(q.copy())
        infos.append(info)
    return np.stack(traj), q, qd, np.stack(infos)


def check_share(info):
    """The reference's own contact set is neither empty nor full, and both branches of the
    Hunt-Crossley clip occur: info [..., P, 2, B] from contact_batch / rollout."""
    info = np.moveaxis(np.asarray(info), -2, 0)  # (f_n, factor) first
    fn, factor = info[0], info[1]
    share = float((fn > 0).mean())
    assert 0.25 <= share <= 0.75, f"active share {share:.3f} outside [0.25, 0.75]"
    pen = ~np.isnan(factor)
    assert (factor[pen] < 0).any(), "the clipped branch (1 + c phid < 0) never occurs"
    assert (factor[pen] > 0).any(), "the unclipped branch never occurs"
    return share


def setup(case, B, seed, **over):
    """(mb with the contact set, mb without, om, m6, cm, inputs) of a named model (ext_wrench_ref.setup);
    the plane's offset is the median height of the set's points over the batch."""
    plain, om, m6 = xr.setup(case)
    q, qd, _, tau, _ = xr.inputs(plain, B, seed)
    links, points = points_for(plain)
    cm = dict(links=links, points=points, normal=NORMAL, **PARAMS)
    cm["offset"] = median_offset(m6, links, points, q, qd)
    cm.update(over)
    mb = plain.with_contacts(cm["links"], cm["points"], normal=cm["normal"], offset=cm["offset"],
                             stiffness=cm["stiffness"], damping=cm["damping"], friction=cm["friction"],
                             slip_velocity=cm["slip_velocity"])
    return mb, plain, om, m6, cm, (q, qd, tau)
