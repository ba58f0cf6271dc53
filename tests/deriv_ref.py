"""Reference for the analytical dynamics derivatives: Richardson-extrapolated central differences of
the fp64 oracle's batched rnea / fd (oracle/oracle.py), the perturbations as extra batch columns so
one oracle call covers every matrix of every configuration.

    D(h) = (f(x + h e_k) - f(x - h e_k)) / 2h        ref = (4 D(h/2) - D(h)) / 3

`consistency` is, per configuration, the largest scaled difference between the extrapolations from
(h, h/2) and from (2h, h): what the reference itself is good for on that input.  rnea is quadratic in qd and
affine in qdd, so any step of order 1 is exact to rounding there; q takes h = 2e-3 rad.
"""
import numpy as np

H_Q = 2e-3
H_V = 0.5


def richardson(f, args, which, h, nthreads=16):
    """d f(*args) / d args[which]: f maps three [n, B] arrays to [n, B].  Returns (ref [n*n, B]
    with row i + n k = d f_i / d x_k, consistency [B])."""
    n, B = args[which].shape
    steps = (2 * h, h, h / 2)
    reps = 2 * len(steps) * n
    big = [np.tile(np.asarray(a, np.float64), (1, reps)) for a in args]
    c = 0
    for s in steps:
        for sign in (1.0, -1.0):
            for k in range(n):
                big[which][k, c * B:(c + 1) * B] += sign * s
                c += 1
    out = f(*big, nthreads=nthreads).reshape(n, len(steps), 2, n, B)  # [i, step, sign, k, b]
    D = [(out[:, t, 0] - out[:, t, 1]) / (2 * s) for t, s in enumerate(steps)]  # [i, k, b]
    ref = (4 * D[2] - D[1]) / 3
    chk = (4 * D[1] - D[0]) / 3
    cons = (np.abs(ref - chk) / (1 + np.abs(ref))).max(axis=(0, 1))
    return np.ascontiguousarray(ref.transpose(1, 0, 2)).reshape(n * n, B), cons


def rnea_deriv_ref(om, q, qd, qdd):
    """(dtau_dq, dtau_dqd) [n*n, B] and the reference's own consistency [B]."""
    dq, c1 = richardson(om.rnea_batch, [q, qd, qdd], 0, H_Q)
    dqd, c2 = richardson(om.rnea_batch, [q, qd, qdd], 1, H_V)
    return dq, dqd, np.maximum(c1, c2)


def fd_deriv_ref(om, q, qd, tau):
    """(dqdd_dq, dqdd_dqd) [n*n, B] by differences of the oracle's forward dynamics, consistency [B]."""
    dq, c1 = richardson(om.fd_batch, [q, qd, tau], 0, H_Q)
    dqd, c2 = richardson(om.fd_batch, [q, qd, tau], 1, H_V)
    return dq, dqd, np.maximum(c1, c2)


def sym_h(om, q):
    """sym(H) [B, n, n] from the oracle's crba (upper triangle, column-major rows)."""
    n, B = q.shape
    H = om.crba_batch(np.asarray(q, np.float64), nthreads=16).reshape(n, n, B).transpose(2, 1, 0)  # [b, row, col]
    U = np.triu(H)
    return U + np.triu(H, 1).transpose(0, 2, 1)


def mats(x):
    """[n*n, B] column-major matrices -> [B, n, n] with [b, i, k]."""
    nn, B = x.shape
    n = int(round(nn ** 0.5))
    return np.asarray(x, np.float64).reshape(n, n, B).transpose(2, 1, 0)


def scaled(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.all(np.isfinite(got)), "non-finite output"
    return float((np.abs(got - ref) / (1 + np.abs(ref))).max())
