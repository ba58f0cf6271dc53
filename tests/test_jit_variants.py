"""Pin of the hipRTC kernel each launch shape takes (CPU only: hipRTC compiles without a device).

tests/golden/jit_variants.json records, for FR3, the 12- and 30-link chains and the 9-joint tree,
under the default tuning and under `pack` 1..5 and `fd_form` 1 / 2, the SHA-1 and length of
Multibody.jit_source(...) and the rbamd::dev:: lane functions the kernel calls.  The points are
tools/gen_jit_variants.py's PLAN (thinned to about a minute of compiles); this test recomputes
them and compares, so a change of the variant resolution or of one character of the generated
source shows here with the names of the lane functions that moved.  It does not reach the
per-device kernel cache (its key and lock-free slot need a device; the GPU suite covers them).

The fixture is regenerated on purpose, by the pull request that changes the kernel policy or
the generated source, never to make a refactor pass.  One input of the source depends on the
compiler, not on this code: a kernel built without an occupancy target that comes out at 257-272
registers is rebuilt with a 2-wave target (jit.hpp, the occupancy cliff), and the source reported
is the rebuilt one; a new ROCm can move a kernel across that edge.
"""
import importlib.util
import json
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _generator():
    spec = importlib.util.spec_from_file_location("gen_jit_variants", os.path.join(REPO, "tools", "gen_jit_variants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_jit_variants_match_fixture():
    with open(os.path.join(REPO, "tests", "golden", "jit_variants.json")) as f:
        want = json.load(f)
    got = _generator().compute()
    assert sorted(got) == sorted(want), "the fixture's points are not the generator's PLAN"
    moved = {k: (want[k]["lanes"], got[k]["lanes"], want[k]["len"], got[k]["len"]) for k in want if got[k] != want[k]}
    assert not moved, f"{len(moved)} of {len(want)} kernels differ (lanes before, after, length before, after): {moved}"
