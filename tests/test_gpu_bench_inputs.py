"""The bench's timed workloads run on valid inputs.  bench.rollout_launcher updates q, qd in
place; without its per-launch reset the state integrated launch after launch diverges to Inf /
NaN (tools/roll_state.py: 95% of FR3 configurations within 200 launches of 16 steps), and the
rollout lines would time a diverged state.  With the reset every launch must leave the same,
finite state, equal to one rollout of the initial draw."""
import pytest

from conftest import PKG, REPO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("B", [1 << 16, 1 << 20])
def test_rollout_launcher_resets_state(dtype, B):
    import sys

    sys.path[:0] = [REPO, PKG]
    import bench
    from rigidbody_amd import ffi

    dt = bench.DT[dtype]
    mb = ffi.Multibody.new()
    mb.upload()
    rl = bench.rollout_launcher(mb, B, dt, 16)
    q, qd, tau, init = rl.keep
    rl(0, None)
    torch.cuda.synchronize()
    first = torch.stack([q, qd]).clone()
    assert torch.isfinite(first).all(), "one 16-step rollout of the bench draw left a non-finite state"
    # the same rollout through the plain binding, from the initial draw
    q1, qd1 = init[0].clone(), init[1].clone()
    mb.rollout_batch(q1, qd1, tau.view(16, mb.n, B), 1e-3)
    torch.cuda.synchronize()
    assert torch.equal(first, torch.stack([q1, qd1]))
    for i in range(1, 40):
        rl(i, None)
    torch.cuda.synchronize()
    assert torch.equal(first, torch.stack([q, qd])), "the launches do not restart from the initial state"
    # reset_only issues the copy alone
    ro = bench.rollout_launcher(mb, B, dt, 16, reset_only=True)
    ro(0, None)
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(ro.keep[:2]), ro.keep[3])


def test_dump_outputs_are_the_last_timed_step(tmp_path):
    """A plain `bench.py --dump-outputs DIR` run (no --full: no CPU baseline, no secondary
    lines) on a ragged batch: DIR/tau.npy and DIR/qdd.npy are [n, B] float64 arrays, bit for bit
    what the timed entry point (multibody_rnea_fd_batch_tiled_f64) gives on the input set of the
    last timed step, that set drawn again here from its seed."""
    import sys

    import numpy as np

    sys.path[:0] = [REPO, PKG]
    from conftest import run_bench
    from rigidbody_amd import chains, ffi
    from rigidbody_amd import dist as rdist

    B, steps = 1000, 3
    out = tmp_path / "out"
    compact, line = run_bench(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--kernel", "rnea_fd",
                               "--batch", str(B), "--spinup-ms", "0", "--rotate-gib", "0.001",
                               "--dump-outputs", str(out)])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and compact["ms_per_step"] == line["ms_per_step"]
    assert "cpu_baseline" not in line and "secondary" not in line
    assert line["dumped_outputs"]["arrays"] == {"tau": [7, B], "qdd": [7, B]}
    ns = line["config"]["input_sets"]
    assert ns > steps  # the last timed step ran on a set of its own, not on set 0
    mb = ffi.Multibody.new()
    mb.upload()
    lim = mb.limits()
    seed = rdist.rank_seed(chains.SEED, 0) + 1000 * ((steps - 1) % ns)
    x = [ffi.to_tiled(ffi.fill_uniform(torch.empty((7, B), dtype=torch.float64, device="cuda"),
                                       *chains.input_ranges(lim, kind), seed + k))
         for k, kind in enumerate(("q", "qd", "qdd", "tau"))]
    want = [ffi.from_tiled(t, B).cpu().numpy() for t in mb.rnea_fd_batch_tiled(*x, B)]
    for name, w in zip(("tau", "qdd"), want):
        got = np.load(out / f"{name}.npy")
        assert got.dtype == np.float64 and got.shape == (7, B)
        assert np.isfinite(got).all()
        np.testing.assert_array_equal(got, w)
