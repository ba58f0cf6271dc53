"""The reverse-mode gradient of the fused rollout on the GPU (multibody_rollout_vjp_batch_*, hipRTC
kind 9, rollout_vjp_body.hip.hpp) and its autograd wrapper.  Inputs and the reference:
rollout_vjp_ref.py; each case is built once per module."""
import ctypes

import numpy as np
import pytest
import torch

import rollout_vjp_ref as ref
from test_deriv_host import _model

pytestmark = pytest.mark.gpu
DT = ref.DT
# host body vs device kernel, fp64: 10x the worst measured, 1.02e-14 (test_parity_with_host_body)
PARITY_BOUND = 1.02e-13
# fp32 kernel vs fp64 kernel on the same fp32-rounded inputs: 4x the worst measured, 9.75e-5 (the
# 12-link chain; FR3 5.1e-6), rounded up (test_fp32_against_fp64)
F32_BOUND = 4e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ffi():
    from rigidbody_amd import ffi

    return ffi


_CASES = {}


def _case(ffi, oracle_mod, name, B, K, f32=False):
    """(mb, om, case): model, oracle and inputs, built once."""
    key = (name, B, K, f32)
    if key not in _CASES:
        mb, om, _ = _CASES.get(name) or _CASES.setdefault(name, _model(ffi, oracle_mod, name))
        _CASES[key] = (mb, om, ref.make_case(om, mb.n, B, K, 8100 + 10 * K + B, f32))
    return _CASES[key]


def _t(c, dev, dtype=torch.float64, cols=None):
    return [torch.as_tensor(np.ascontiguousarray(c[k][..., :cols] if cols else c[k]), device=dev).to(dtype)
            for k in ("q", "qd", "tau", "gq", "gqd")]


def _run(mb, x):
    return mb.rollout_vjp_batch(x[0], x[1], x[2], DT, x[3], x[4])


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("B", [257, 1])
def test_parity_with_host_body(ffi, oracle_mod, dev, B, K):
    """Every configuration against the single-configuration host body (the same lane code under the
    host compiler), FR3 fp64, relative to the largest element of each output array of the
    configuration.  One evaluation of one body under two compilers agrees to 1e-12 in this project;
    K chained steps compound it.  Measured on the MI355X: B = 257 K = 1 8.8e-15, K = 3 1.02e-14; B = 1
    2.4e-15 / 6.0e-16.  PARITY_BOUND is 10x the worst, 1.02e-13; a value above 1e-9 would be a finding,
    not a tolerance to widen."""
    mb, om, c = _case(ffi, oracle_mod, "fr3", 257, K)
    got = [g.cpu().numpy() for g in _run(mb, _t(c, dev, cols=B))]
    worst = 0.0
    for b in range(B):
        want = mb.rollout_vjp(c["q"][:, b], c["qd"][:, b], c["tau"][:, :, b], DT, c["gq"][:, :, b], c["gqd"][:, :, b])
        for g, w in zip(got, want):
            assert np.all(np.isfinite(g[..., b]))
            worst = max(worst, np.abs(g[..., b] - w).max() / np.abs(w).max())
    print(f"host parity B={B} K={K}: worst relative difference {worst:.3e}")
    assert worst <= PARITY_BOUND


@pytest.mark.parametrize("name,B", [("fr3", 300), ("chain12", 300), ("general7", 20)])
def test_parity_with_reference(ffi, oracle_mod, dev, name, B):
    """The first 20 configurations against the oracle's directional derivative, with the CPU test's
    tolerance and qualification rule."""
    mb, om, c = _case(ffi, oracle_mod, name, B, 3)
    got = [g.cpu().numpy()[..., :20] for g in _run(mb, _t(c, dev))]
    c20 = {k: np.ascontiguousarray(v[..., :20]) for k, v in c.items()}
    want, cons = ref.directional(om, c20)
    good = cons <= 1e-8
    err = np.abs(ref.pairing(got, (c20["dq"], c20["dqd"], c20["dtau"])) - want) / (1 + np.abs(want))
    print(f"{name}: {int(good.sum())} of 20 references within 1e-8; worst error on them {err[good].max():.2e}")
    assert good.sum() >= (15 if name == "chain12" else 20)
    assert err[good].max() <= 1e-7


@pytest.mark.parametrize("name", ["fr3", "chain12"])
def test_fp32_against_fp64(ffi, oracle_mod, dev, name):
    """fp32 kernel against the fp64 kernel on the same fp32-rounded inputs, B = 257, K = 3: per
    output array and configuration max|d| / (1 + max|ref|).  Measured on the MI355X: FR3 5.06e-6, the
    12-link chain 9.74e-5.  F32_BOUND is 4x the worst, rounded up: 4e-4 (the convention for the fp32
    derivative bounds; rigidbody_batch.h states it)."""
    mb, om, c = _case(ffi, oracle_mod, name, 257, 3, True)
    g64 = _run(mb, _t(c, dev))
    g32 = _run(mb, _t(c, dev, torch.float32))
    worst = 0.0
    for a, b in zip(g32, g64):
        a, b = a.double().reshape(-1, 257), b.reshape(-1, 257)
        assert bool(torch.isfinite(a).all())
        worst = max(worst, float(((a - b).abs().amax(0) / (1 + b.abs().amax(0))).max()))
    print(f"{name} fp32 vs fp64: worst {worst:.3e}")
    assert worst <= F32_BOUND


def _raw(ffi, mb, x, B, ld, K, outs):
    fn = ffi.lib().multibody_rollout_vjp_batch_f64
    rc = fn(mb.handle, x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), DT, K, x[3].data_ptr(), x[4].data_ptr(),
            *[o.data_ptr() for o in outs], B, ld, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, ffi.last_error()


def test_leading_dimension(ffi, oracle_mod, dev):
    """ld = 260 > B = 257: bit-identical to the contiguous call, padding columns untouched."""
    mb, om, c = _case(ffi, oracle_mod, "fr3", 257, 3)
    n, K, B, ld = mb.n, 3, 257, 260
    x = _t(c, dev)
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


def test_domain(ffi, oracle_mod, dev):
    """A NaN in the last step's torques, an angle past the bound in q: every output of those
    configurations is NaN (g_tau of the earlier steps too), their neighbours unchanged."""
    mb, om, c = _case(ffi, oracle_mod, "fr3", 257, 3)
    x = _t(c, dev)
    clean = _run(mb, x)
    x[2] = x[2].clone()
    x[0] = x[0].clone()
    x[2][2, 4, 17] = float("nan")
    x[0][5, 200] = 2.0 ** 42
    bad = [17, 200]
    good = torch.ones(257, dtype=torch.bool, device=dev)
    good[bad] = False
    for got, want in zip(_run(mb, x), clean):
        assert bool(torch.isnan(got[..., bad]).all())
        assert torch.equal(got[..., good], want[..., good])


def test_host_pointer_form(ffi, oracle_mod, dev):
    mb, om, c = _case(ffi, oracle_mod, "fr3", 257, 3)
    want = _run(mb, _t(c, dev))
    got = mb.rollout_vjp_batch_host(c["q"], c["qd"], c["tau"], DT, c["gq"], c["gqd"])
    for g, w in zip(got, want):
        assert np.array_equal(g, w.cpu().numpy())


def test_graph_capture(ffi, oracle_mod, dev):
    mb, om, c = _case(ffi, oracle_mod, "fr3", 1000, 3)
    mb.upload()
    x = _t(c, dev)
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


def test_autograd_gradcheck(ffi, oracle_mod, dev):
    """torch.autograd.gradcheck with its default tolerances: the numerical side is the existing
    rollout kernel, the analytical side one rollout_vjp_batch launch per output cotangent."""
    from rigidbody_amd import autograd

    mb, om, c = _case(ffi, oracle_mod, "fr3", 2, 2)
    q0, qd0, tau = (t.requires_grad_(True) for t in _t(c, dev)[:3])
    assert torch.autograd.gradcheck(lambda a, b, t: autograd.rollout(mb, a, b, t, DT), (q0, qd0, tau))
