"""The reverse-mode gradient of the fused contact rollout on the GPU
(multibody_rollout_contact_vjp_batch_*, contact_vjp_body.hip.hpp) and its autograd wrapper.  Inputs,
the reference and the qualification rule: contact_vjp_ref.py; each case is built once per session."""
import ctypes

import numpy as np
import pytest
import torch

import contact_vjp_ref as ref
import rollout_vjp_ref as rv

pytestmark = pytest.mark.gpu
DT = ref.DT
B = 257
# host body vs device kernel, fp64: 10x the worst measured (test_parity_with_host_body)
PARITY_BOUND = 7.02e-13
# fp32 kernel vs fp64 kernel on the same fp32-rounded inputs, away from the law's kinks: 4x the worst
# measured, rounded up (test_fp32_against_fp64)
F32_BOUND = 6e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ffi():
    from rigidbody_amd import ffi

    return ffi


def _t(c, dev, dtype=torch.float64, cols=None):
    return [torch.as_tensor(np.ascontiguousarray(c[k][..., :cols] if cols else c[k]), device=dev).to(dtype)
            for k in ("q", "qd", "tau", "gq", "gqd")]


def _run(mb, x):
    return mb.rollout_contact_vjp_batch(x[0], x[1], x[2], DT, x[3], x[4])


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("cols", [257, 1])
def test_parity_with_host_body(ffi, dev, cols, K):
    """Every configuration against the single-configuration host body (the same lane code under the
    host compiler), FR3 fp64, relative to the largest element of each output array of the
    configuration.  Measured on the MI355X: B = 257 K = 1 2.5e-14, K = 3 7.01e-14; B = 1
    4.2e-15 / 1.6e-15.  PARITY_BOUND is 10x the worst, 7.02e-13; a value above 1e-9 would be a finding, not a
    tolerance to widen."""
    cs = ref.case("fr3", B, K)
    mb, c = cs["mb"], cs["c"]
    got = [g.cpu().numpy() for g in _run(mb, _t(c, dev, cols=cols))]
    # The plane sits at the median of an odd number (3 x 257) of point heights: exactly at one point of
    # one configuration, whose branch of max(gap, 0) is decided by the last bit of x_p -- two compilers'
    # roundings may differ there (measured: that configuration's g_q0 alone, 0.24 relative).  It is
    # not compared; by construction there is one, and no more than one is let through.
    on_plane = ref.near_kink(cs, height=1e-12, factor=0.0)
    assert on_plane.sum() <= 1
    worst = 0.0
    for b in np.flatnonzero(~on_plane[:cols]):
        want = mb.rollout_contact_vjp(c["q"][:, b], c["qd"][:, b], c["tau"][:, :, b], DT, c["gq"][:, :, b],
                                      c["gqd"][:, :, b])
        for g, w in zip(got, want):
            assert np.all(np.isfinite(g[..., b]))
            worst = max(worst, np.abs(g[..., b] - w).max() / np.abs(w).max())
    print(f"host parity B={cols} K={K}: worst relative difference {worst:.3e}")
    assert worst <= PARITY_BOUND


@pytest.mark.parametrize("name", ["fr3", "chain12", "general7"])
def test_parity_with_reference(ffi, dev, name):
    """The first 40 of 257 configurations against the reference's directional derivative, with the CPU
    test's tolerance and qualification rule; the reference's active share inside its band."""
    cs = ref.case(name, B)
    assert 0.25 <= cs["share"] <= 0.75
    got = [g.cpu().numpy()[..., :ref.NCFG] for g in _run(cs["mb"], _t(cs["c"], dev))]
    ref.check(got, cs, cols=ref.NCFG, label=name)


class _GpuStepper:
    """One step of multibody_rollout_contact_batch_f64 behind rollout_vjp_ref.trajectory's call."""

    def __init__(self, mb, dev):
        self.mb, self.dev = mb, dev

    def rollout_batch(self, q, qd, tau_seq, dt, nthreads=1):
        q, qd, tau = (torch.as_tensor(np.ascontiguousarray(a), device=self.dev) for a in (q, qd, tau_seq))
        self.mb.rollout_contact_batch(q, qd, tau, dt)
        return q.cpu().numpy(), qd.cpu().numpy(), None


def test_against_differences_of_the_gpu_rollout(ffi, dev):
    """FR3 (the mass-matrix form in both kernels): the gradient paired with a direction against
    Richardson differences of multibody_rollout_contact_batch_f64 itself, the first 40 configurations,
    the same qualification rule and tolerance."""
    cs = ref.case("fr3", B)
    c = {k: np.ascontiguousarray(v[..., :ref.NCFG]) for k, v in cs["c"].items()}
    want, cons = rv.directional(_GpuStepper(cs["mb"], dev), c, dt=DT, h=ref.H)
    got = [g.cpu().numpy()[..., :ref.NCFG] for g in _run(cs["mb"], _t(cs["c"], dev))]
    good = cons <= ref.CONS
    err = np.abs(rv.pairing(got, (c["dq"], c["dqd"], c["dtau"])) - want) / (1 + np.abs(want))
    print(f"fr3 vs differences of the GPU rollout: {int(good.sum())} of {good.size} qualify; worst error on them "
          f"{err[good].max():.2e}")
    assert good.sum() >= ref.MIN_GOOD
    assert err[good].max() <= ref.TOL


@pytest.mark.parametrize("name", ["fr3", "chain12"])
def test_fp32_against_fp64(ffi, dev, name):
    """fp32 kernel against the fp64 kernel on the same fp32-rounded inputs, B = 257, K = 3: per output
    array and configuration max|d| / (1 + max|ref|).  Configurations whose fp64 reference trajectory
    comes within 1e-3 m of the plane at any (point, step), or has |1 + c phid| < 1e-2 while penetrating,
    are excluded -- a rounding flip of the branch there is not an error; at least 80% must remain
    (asserted on the reference).  Measured on the MI355X: FR3 2.01e-5 with 251 of 257 kept, the 12-link chain
    1.47e-4 with 256 kept.  F32_BOUND is 4x the worst, rounded up: 6e-4 (rigidbody_batch.h states it)."""
    cs = ref.case(name, B, f32=True)
    keep = ~ref.near_kink(cs)
    print(f"{name}: {int(keep.sum())} of {B} configurations away from the kinks")
    assert keep.sum() >= 0.8 * B
    g64 = _run(cs["mb"], _t(cs["c"], dev))
    g32 = _run(cs["mb"], _t(cs["c"], dev, torch.float32))
    keep_t = torch.as_tensor(keep, device=dev)
    worst = 0.0
    for a, b in zip(g32, g64):
        a, b = a.double().reshape(-1, B)[:, keep_t], b.reshape(-1, B)[:, keep_t]
        assert bool(torch.isfinite(a).all())
        worst = max(worst, float(((a - b).abs().amax(0) / (1 + b.abs().amax(0))).max()))
    print(f"{name} fp32 vs fp64: worst {worst:.3e}")
    assert worst <= F32_BOUND


def _raw(ffi, mb, x, batch, ld, K, outs):
    fn = ffi.lib().multibody_rollout_contact_vjp_batch_f64
    rc = fn(mb.handle, x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), DT, K, x[3].data_ptr(), x[4].data_ptr(),
            *[o.data_ptr() for o in outs], batch, ld, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, ffi.last_error()


def test_leading_dimension(ffi, dev):
    """ld = 260 > B = 257: bit-identical to the contiguous call, padding columns untouched."""
    cs = ref.case("fr3", B)
    mb = cs["mb"]
    n, K, ld = mb.n, ref.K, 260
    x = _t(cs["c"], dev)
    want = _run(mb, x)
    wide = []
    for t in x:
        w = torch.full((t.numel() // B, ld), -7.0, dtype=torch.float64, device=dev)
        w[:, :B] = t.reshape(-1, B)
        wide.append(w)
    outs = [torch.full((rows, ld), -7.0, dtype=torch.float64, device=dev) for rows in (n, n, K * n, 2 * K * n)]
    _raw(ffi, mb, wide, B, ld, K, outs)
    torch.cuda.synchronize(dev)
    for o, w in zip(outs[:3], want):
        assert torch.equal(o[:, :B], w.reshape(-1, B))
        assert bool((o[:, B:] == -7.0).all())
    assert bool((outs[3][:, B:] == -7.0).all())  # nor does the workspace reach past the batch


def test_domain(ffi, dev):
    """A NaN in the last step's torques, an angle of 2^42 in q: every output of those configurations
    is NaN (g_tau of the earlier steps too), their neighbours bit-identical."""
    cs = ref.case("fr3", B)
    mb = cs["mb"]
    x = _t(cs["c"], dev)
    clean = _run(mb, x)
    x[2] = x[2].clone()
    x[0] = x[0].clone()
    x[2][2, 4, 17] = float("nan")
    x[0][5, 200] = 2.0 ** 42
    bad = [17, 200]
    good = torch.ones(B, dtype=torch.bool, device=dev)
    good[bad] = False
    for got, want in zip(_run(mb, x), clean):
        assert bool(torch.isnan(got[..., bad]).all())
        assert torch.equal(got[..., good], want[..., good])


def test_host_pointer_form(ffi, dev):
    cs = ref.case("fr3", B)
    c = cs["c"]
    want = _run(cs["mb"], _t(c, dev))
    got = cs["mb"].rollout_contact_vjp_batch_host(c["q"], c["qd"], c["tau"], DT, c["gq"], c["gqd"])
    for g, w in zip(got, want):
        assert np.array_equal(g, w.cpu().numpy())


def test_graph_capture(ffi, dev):
    cs = ref.case("fr3", B)
    mb = cs["mb"]
    mb.upload()
    x = _t(cs["c"], dev)
    eager = _run(mb, x)  # compiles the kernel outside the capture
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _run(mb, x)
    for o in out:
        o.zero_()
    g.replay()
    torch.cuda.synchronize(dev)
    for o, e in zip(out, eager):
        assert torch.equal(o, e)


def test_autograd_gradcheck(ffi, dev):
    """torch.autograd.gradcheck with its default tolerances on two qualified FR3 configurations,
    K = 2: the numerical side is the rollout_contact kernel, the analytical side one
    rollout_contact_vjp_batch launch per output cotangent; the values are autograd.rollout's."""
    from rigidbody_amd import autograd

    cs = ref.case("fr3", ref.NCFG, 2)
    _, cons = ref.directional(cs)
    pick = np.flatnonzero(cons <= ref.CONS)[:2]
    assert pick.size == 2
    c = {k: np.ascontiguousarray(v[..., pick]) for k, v in cs["c"].items()}
    q0, qd0, tau = (t.requires_grad_(True) for t in _t(c, dev)[:3])
    traj, qd_final = autograd.rollout_contact(cs["mb"], q0, qd0, tau, DT)
    q, qd = q0.detach().clone(), qd0.detach().clone()
    assert torch.equal(traj, cs["mb"].rollout_contact_batch(q, qd, tau.detach(), DT)) and torch.equal(qd_final, qd)
    assert torch.autograd.gradcheck(lambda a, b, t: autograd.rollout_contact(cs["mb"], a, b, t, DT), (q0, qd0, tau))
