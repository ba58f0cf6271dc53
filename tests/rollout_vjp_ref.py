"""Reference for the gradient of the fused rollout (multibody_rollout_vjp*): the fp64 oracle's own
rollout, every intermediate (q, qd) from K one-step oracle.rollout_batch calls, the scalar

    L = sum_k gq[k] . q_{k+1} + gqd[k] . qd_{k+1}

and its directional derivative along (dq0, dqd0, dtau) by Richardson central differences,

    D(s) = (L(x + s d) - L(x - s d)) / 2s        ref = (4 D(h/2) - D(h)) / 3,   h = 2e-3

`consistency` is, per configuration, the scaled difference between the extrapolations from (h, h/2)
and from (2h, h), as deriv_ref.richardson: what the reference is good for on that input.

Inputs (make_case): q ~ U(-2, 2), qd ~ U(-1, 1), tau_k = rnea(q, qd, qdd_k) with qdd_k ~ U(-3, 3) so
the motion stays tame, standard-normal cotangents, a random direction of unit Euclidean norm (h is
then a step length in input space, as deriv_ref's steps along unit vectors), dt = 0.01; fp32 cases round every
input to fp32 first.
"""
import numpy as np

H = 2e-3
DT = 0.01


def make_case(om, n, B, K, seed, f32=False):
    rng = np.random.default_rng(seed)
    q, qd = rng.uniform(-2, 2, (n, B)), rng.uniform(-1, 1, (n, B))
    tau = np.stack([om.rnea_batch(q, qd, rng.uniform(-3, 3, (n, B))) for _ in range(K)])
    c = dict(q=q, qd=qd, tau=tau, gq=rng.standard_normal((K, n, B)), gqd=rng.standard_normal((K, n, B)),
             dq=rng.standard_normal((n, B)), dqd=rng.standard_normal((n, B)), dtau=rng.standard_normal((K, n, B)))
    # a unit direction per configuration, so that h is a step length in input space as in deriv_ref
    norm = np.sqrt((c["dq"] ** 2).sum(0) + (c["dqd"] ** 2).sum(0) + (c["dtau"] ** 2).sum((0, 1)))
    for k in ("dq", "dqd", "dtau"):
        c[k] = c[k] / norm
    if f32:
        c = {k: v.astype(np.float32).astype(np.float64) for k, v in c.items()}
    return c


def trajectory(om, q, qd, tau_seq, dt=DT):
    """(q_{k+1}, qd_{k+1}) for k < K, each [K, n, B]."""
    qs, vs = [], []
    for k in range(tau_seq.shape[0]):
        q, qd, _ = om.rollout_batch(q, qd, tau_seq[k:k + 1], dt, nthreads=16)
        qs.append(q)
        vs.append(qd)
    return np.stack(qs), np.stack(vs)


def loss(om, c, q, qd, tau, dt=DT):
    """L per configuration [B] (the cotangents tiled when q carries repeated blocks of them)."""
    qs, vs = trajectory(om, q, qd, tau, dt)
    reps = q.shape[1] // c["gq"].shape[2]
    return (np.tile(c["gq"], (1, 1, reps)) * qs + np.tile(c["gqd"], (1, 1, reps)) * vs).sum(axis=(0, 1))


def directional(om, c, direction=None, dt=DT, h=H):
    """(ref [B], consistency [B]) of dL along direction = (dq0, dqd0, dtau) (default: the case's)."""
    dq, dqd, dtau = direction if direction is not None else (c["dq"], c["dqd"], c["dtau"])
    B = c["q"].shape[1]
    steps = (2 * h, h, h / 2)
    signed = [sg * s for s in steps for sg in (1.0, -1.0)]
    q = np.concatenate([c["q"] + s * dq for s in signed], axis=1)
    qd = np.concatenate([c["qd"] + s * dqd for s in signed], axis=1)
    tau = np.concatenate([c["tau"] + s * dtau for s in signed], axis=2)
    L = loss(om, c, q, qd, tau, dt).reshape(len(steps), 2, B)
    D = [(L[t, 0] - L[t, 1]) / (2 * s) for t, s in enumerate(steps)]
    ref = (4 * D[2] - D[1]) / 3
    chk = (4 * D[1] - D[0]) / 3
    return ref, np.abs(ref - chk) / (1 + np.abs(ref))


def pairing(g, direction):
    """<(g_q0, g_qd0, g_tau), (dq0, dqd0, dtau)> per configuration; the arrays [n, B] / [K, n, B]."""
    return (g[0] * direction[0]).sum(axis=0) + (g[1] * direction[1]).sum(axis=0) + (g[2] * direction[2]).sum(axis=(0, 1))
