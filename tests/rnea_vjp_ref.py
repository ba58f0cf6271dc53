"""Reference for the reverse-mode gradient of the inverse dynamics (rnea_vjp), built on
tests/ext_wrench_ref.py:

    tau_ref(q, qd, qdd, fext) = om.rnea_batch(q, qd, qdd) - jt_f_batch(m6, q, fext)

For a direction d = (dq, dqd, dqdd, dfext), each block scaled to its input's range, the reference
value of <g, d> is the Richardson-extrapolated central difference of w . tau_ref along d.  tau is
affine in qdd and fext and quadratic in qd, so only the q block limits the reference: its
truncation error after one extrapolation is O(h^4).  Two step pairs (H, H/2) and (H/2, H/4) give a
self-consistency estimate per configuration; a configuration counts only where they agree to
QUALIFY (relative), and at most MAX_LEFT_OUT of a batch may be left out.  H = 1e-3 (times half
ranges of up to pi rad) keeps the truncation and the rounding of the differences (1e-16 |L| / h)
near 1e-10; on the CPU every configuration of every model in the tests qualifies.
Shared by tests/test_rnea_vjp_host.py and tests/test_gpu_rnea_vjp.py.
"""
import numpy as np

from ext_wrench_ref import FORCE, MOMENT, inputs, jt_f_batch, setup  # noqa: F401  (re-exported)

H = 1e-3
QUALIFY = 1e-8
MAX_LEFT_OUT = 0.10
BOUND = 1e-7  # |<g, d> - ref| <= BOUND (1 + |ref|)


def tau_ref(om, m6, q, qd, qdd, fext):
    tau = om.rnea_batch(q, qd, qdd)
    return tau if fext is None else tau - jt_f_batch(m6, q, fext)


def cotangent(mb, B, seed):
    """w [n, B], uniform in +-1."""
    return 2.0 * np.random.default_rng(seed).random((mb.n, B)) - 1.0


def direction(mb, B, seed, with_fext):
    """(dq, dqd, dqdd, dfext or None): uniform in +-1 times each input's half range."""
    from rigidbody_amd import chains

    lim = mb.limits()
    rng = np.random.default_rng(seed)
    out = []
    for kind in ("q", "qd", "qdd"):
        lo, hi = (np.asarray(x, float) for x in chains.input_ranges(lim, kind))
        out.append(0.5 * (hi - lo)[:, None] * (2.0 * rng.random((mb.n, B)) - 1.0))
    amp = np.tile([FORCE] * 3 + [MOMENT] * 3, mb.n)[:, None]
    out.append(amp * (2.0 * rng.random((6 * mb.n, B)) - 1.0) if with_fext else None)
    return out


def directional(om, m6, q, qd, qdd, fext, w, d):
    """(ref [B], err [B]): the Richardson central difference of w . tau_ref along d, and the relative
    disagreement of the two step pairs."""
    dq, dqd, dqdd, dfext = d

    def L(t):
        f = None if fext is None else fext + t * dfext
        return np.sum(w * tau_ref(om, m6, q + t * dq, qd + t * dqd, qdd + t * dqdd, f), axis=0)

    def central(h):
        return (L(h) - L(-h)) / (2.0 * h)

    c1, c2, c4 = central(H), central(H / 2), central(H / 4)
    coarse = (4.0 * c2 - c1) / 3.0
    fine = (4.0 * c4 - c2) / 3.0
    return fine, np.abs(fine - coarse) / (1.0 + np.abs(fine))


def contract(g, d):
    """<g, d> per configuration: g = (g_q, g_qd, g_qdd[, g_fext]) arrays [rows, B]."""
    return sum(np.sum(np.asarray(a, float) * b, axis=0) for a, b in zip(g, d) if b is not None)


def check_parity(got, ref, err, what=""):
    """The qualifying rule and the bound; returns the measured maximum."""
    ok = err <= QUALIFY
    assert ok.mean() >= 1.0 - MAX_LEFT_OUT, f"{what}: only {ok.sum()} of {ok.size} configurations qualify"
    rel = np.abs(got - ref)[ok] / (1.0 + np.abs(ref[ok]))
    print(f"rnea_vjp parity {what}: max {rel.max():.3e} ({ok.sum()} of {ok.size} qualify, self-consistency "
          f"{err[ok].max():.1e})")
    assert rel.max() <= BOUND, f"{what}: {rel.max():.3e}"
    return rel.max()


def scaled(a, b):
    """max|a - b| / (1 + max|b|)."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / (1.0 + np.abs(b).max())
