"""Reference for the gradient of the fused contact rollout (multibody_rollout_contact_vjp*), numpy fp64.

The rollout is assembled per step from the reference contact law, the oracle's forward dynamics and
the semi-implicit Euler update (contact_ref.rollout's step; that function does not return the
velocities after each step, which the loss needs):

    fext = contact_ref.contact_batch(q, qd)     a = om.fd_batch(q, qd, tau + J^T fext)
    qd' = qd + dt a                              q' = q + dt qd'
    L = sum_k gq[k] . q_{k+1} + gqd[k] . qd_{k+1}

and differentiated along a unit direction by rollout_vjp_ref.directional -- Richardson central
differences, h = 2e-3, with its consistency measure -- through a stepper object that stands in for the
oracle model there.

Inputs (case): rollout_vjp_ref.make_case's (q ~ U(-2, 2), qd ~ U(-1, 1), tau_k = rnea(q, qd, U(-3, 3)),
standard-normal cotangents, a unit direction), contact_ref.points_for's set with contact_ref.PARAMS,
the plane at the median point height of the batch, dt = 1e-3, K = 3.

Qualification: a configuration counts where the reference is self-consistent to CONS (1e-8) -- the ones
that cross a kink of the law within the differencing step are not -- and at least MIN_GOOD of NCFG
must.  `case` also asserts contact_ref.check_share's active band on the reference trajectory, so no
user can pass on a contact-free batch.  Shared by tests/test_contact_vjp_host.py and
tests/test_gpu_contact_vjp.py; every case is built once (cached).
"""
import numpy as np

import contact_ref as cr
import ext_wrench_ref as xr
import rollout_vjp_ref as rv

H = 2e-3
DT = cr.DT
K = 3
NCFG = 40
MIN_GOOD = 32
CONS = 1e-8
TOL = 1e-7  # |<g, d> - ref| <= TOL (1 + |ref|): rollout_vjp's contract


class Stepper:
    """One contact-rollout step behind the oracle model's rollout_batch signature, as
    rollout_vjp_ref.trajectory calls it (one step at a time)."""

    def __init__(self, om, m6, cm):
        self.om, self.m6, self.cm = om, m6, cm

    def step(self, q, qd, tau, dt):
        fext, _, info = cr.contact_batch(self.m6, self.cm, q, qd)
        a = self.om.fd_batch(q, qd, tau + xr.jt_f_batch(self.m6, q, fext))
        qd = qd + dt * a
        return q + dt * qd, qd, info

    def rollout_batch(self, q, qd, tau_seq, dt, nthreads=1):
        assert tau_seq.shape[0] == 1
        return self.step(np.asarray(q, float), np.asarray(qd, float), tau_seq[0], dt)


def trajectory_info(st, c, dt=DT):
    """(info [K, P, 2, B], gap [K, P, B]) of the case's own trajectory: contact_ref's (f_n, 1 + c phid) and
    d - nhat . x_p of every point before every step."""
    q, qd = c["q"], c["qd"]
    cm, nh = st.cm, np.asarray(st.cm["normal"], float)
    infos, gaps = [], []
    for tau in c["tau"]:
        gaps.append(np.stack([cm["offset"] - cr.point_kin(st.m6, cm["links"], cm["points"], q[:, b], qd[:, b])[0] @ nh
                              for b in range(q.shape[1])], axis=-1))
        q, qd, info = st.step(q, qd, tau, dt)
        infos.append(info)
    return np.stack(infos), np.stack(gaps)


_CASES = {}
_MODELS = {}


def model(name):
    """(plain Multibody, oracle model, Model6), built once."""
    if name not in _MODELS:
        _MODELS[name] = xr.setup(name)
    return _MODELS[name]


def contact_model(name, q, qd, **over):
    """(mb with the test contact set, cm): the plane at the median point height of (q, qd)."""
    plain, om, m6 = model(name)
    links, points = cr.points_for(plain)
    cm = dict(links=links, points=points, normal=cr.NORMAL, **cr.PARAMS)
    cm["offset"] = cr.median_offset(m6, links, points, q, qd)
    cm.update(over)
    mb = plain.with_contacts(cm["links"], cm["points"], normal=cm["normal"], offset=cm["offset"],
                             stiffness=cm["stiffness"], damping=cm["damping"], friction=cm["friction"],
                             slip_velocity=cm["slip_velocity"])
    return mb, cm


def case(name, B=NCFG, k=K, seed=9100, f32=False, **over):
    """dict(mb, plain, st, cm, c, share): model with the contact set, the plain model, the reference
    stepper, the contact model, rollout_vjp_ref's inputs, and the reference's active share (asserted
    inside check_share's band)."""
    key = (name, B, k, seed, f32, tuple(sorted(over.items())))
    if key not in _CASES:
        plain, om, m6 = model(name)
        c = rv.make_case(om, plain.n, B, k, seed + 10 * k + B, f32)
        mb, cm = contact_model(name, c["q"], c["qd"], **over)
        st = Stepper(om, m6, cm)
        info, gap = trajectory_info(st, c)
        # (the cases that switch the contact off on purpose have no share to assert)
        share = cr.check_share(info) if cm["stiffness"] > 0 and "offset" not in over else None
        _CASES[key] = dict(mb=mb, plain=plain, st=st, cm=cm, c=c, share=share, info=info, gap=gap)
    return _CASES[key]


def directional(cs, cols=None):
    """(ref [B], consistency [B]) of the case's first `cols` configurations, cached."""
    key = ("dir", cols)
    if key not in cs:
        c = cs["c"] if cols is None else {k: np.ascontiguousarray(v[..., :cols]) for k, v in cs["c"].items()}
        cs[key] = rv.directional(cs["st"], c, dt=DT, h=H)
    return cs[key]


def check(got, cs, cols=None, label=""):
    """Assert the directional pairing of `got` = (g_q0, g_qd0, g_tau) (first `cols` configurations)
    against the reference under the qualification rule; returns (qualified, worst error on them)."""
    c = cs["c"] if cols is None else {k: v[..., :cols] for k, v in cs["c"].items()}
    want, cons = directional(cs, cols)
    good = cons <= CONS
    err = np.abs(rv.pairing(got, (c["dq"], c["dqd"], c["dtau"])) - want) / (1 + np.abs(want))
    print(f"{label}: {int(good.sum())} of {good.size} references within {CONS:g} (median consistency "
          f"{np.median(cons):.2e}); worst error on them {err[good].max():.2e}, on all {err.max():.2e}")
    assert good.sum() >= MIN_GOOD * good.size // NCFG
    assert err[good].max() <= TOL
    return int(good.sum()), float(err[good].max())


def near_kink(cs, height=1e-3, factor=1e-2):
    """Per configuration [B]: True where the reference trajectory has a (point, step) within `height`
    metres of the plane, or, while penetrating, |1 + c phid| < factor -- where rounding may flip a
    branch of the law."""
    near = (np.abs(cs["gap"]) < height).any(axis=(0, 1))
    fac = cs["info"][:, :, 1, :]  # NaN where the point does not penetrate
    return near | (np.abs(fac) < factor).any(axis=(0, 1))
