"""Generate tests/golden/jit_variants.json: which hipRTC kernel source each launch shape takes.

For every point (model, tuning state, kind, dtype, batch, layout) the fixture records the SHA-1
and length of Multibody.jit_source(...) and the rbamd::dev:: lane functions the kernel calls (the
names make a diff readable).  tests/test_jit_variants.py recomputes and compares.

Run it against the library whose behaviour is to be pinned (RIGIDBODY_AMD_LIB selects one), and
only on purpose: a pull request that changes the kernel policy regenerates the fixture and says
so; a refactor must pass with the fixture untouched.

    python tools/gen_jit_variants.py            # rewrites tests/golden/jit_variants.json
"""
import hashlib
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "rigidbody-rs_amd"))

from rigidbody_amd import chains, ffi  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "jit_variants.json")

MODELS = {
    "fr3": lambda: ffi.Multibody.new(),
    "chain12": lambda: ffi.Multibody.from_urdf_string(chains.synthetic_chain_urdf(12)),
    "chain30": lambda: ffi.Multibody.from_urdf_string(chains.synthetic_chain_urdf(30)),
    "tree9": lambda: ffi.Multibody.from_urdf_string(chains.tree_urdf(), ffi.URDF_TREE | ffi.GENERAL_AXES),
}
ALL_KINDS = ("rnea", "fd", "crba", "rollout", "fwd_kin", "jac", "rnea_fd")
BOTH = (False, True)
# each side of the batch thresholds of the auto policy; the big launch on the tiled layout
SHAPES = ((1 << 16, False), ((1 << 17) + 1, False), (1 << 20, True))
BIG = ((1 << 20, True),)
# Every point costs a hipRTC compile (0.3-0.8 s for FR3, up to 8 s for a 30-link forward
# dynamics), so the full cross product (17 minutes) is thinned to about a minute.  FR3 carries
# the batch thresholds (the kinds that have one, at every shape) and every tuning state on the
# kinds and dtypes that state can change.  The other models carry their own policy edges (12
# links: mass-matrix FD but ABA rollout; 30 links: the parked / reversed RNEA and the fused
# kind's source no launch takes; the tree: tree forms) and, under the non-default states, the
# points where a requested lane form is clamped to what the model allows.
# (model, tuning key, value, kinds, dtypes, shapes)
F32 = (False,)
PLAN = [("fr3", None, None, ("rnea", "fd", "rollout", "rnea_fd"), BOTH, SHAPES),
        ("fr3", None, None, ("crba", "fwd_kin", "jac"), BOTH, BIG)]
for _v in (1, 2, 3, 4, 5):
    PLAN += [("fr3", "pack", _v, ("fd", "rollout", "rnea_fd"), F32, BIG), ("fr3", "pack", _v, ("rnea",), (True,), BIG)]
for _v in (1, 2):
    PLAN += [("fr3", "fd_form", _v, ("fd", "rollout", "rnea_fd"), F32, BIG)]
PLAN += [("chain12", None, None, ("rnea", "fd", "rollout", "rnea_fd"), BOTH, BIG),
         ("chain30", None, None, ("rnea", "rnea_fd"), BOTH, BIG),
         ("tree9", None, None, ("rnea",), BOTH, BIG),
         ("tree9", None, None, ("fd", "fwd_kin"), F32, BIG)]
for _v in (2, 3, 4, 5):
    PLAN += [("chain12", "pack", _v, ("fd",), F32, BIG), ("tree9", "pack", _v, ("fd",), F32, BIG)]
PLAN += [("chain12", "pack", 2, ("rollout",), F32, BIG), ("chain12", "pack", 4, ("rollout",), F32, BIG),
         ("tree9", "pack", 4, ("rollout",), F32, BIG),
         ("chain30", "pack", 3, ("rnea",), F32, BIG),
         ("chain30", "pack", 5, ("rnea_fd",), F32, BIG), ("tree9", "pack", 5, ("rnea_fd",), F32, BIG),
         ("chain12", "fd_form", 1, ("fd", "rnea_fd"), F32, BIG),
         ("chain30", "fd_form", 1, ("rnea_fd",), F32, BIG),  # (fd_form 2 on 30 links compiles for two minutes)
         ("tree9", "fd_form", 2, ("fd", "rnea_fd"), F32, BIG)]


def record(src):
    kernel = src[src.index("rb_jit_kernel("):]
    return {"sha1": hashlib.sha1(src.encode()).hexdigest(), "len": len(src),
            "lanes": sorted(set(re.findall(r"rbamd::dev::(\w+)<", kernel)))}


def points():
    """(model name, tuning key, value, kind, f64, batch, tiled), grouped by model and state."""
    for name, key, value, kinds, dtypes, shapes in PLAN:
        for kind in kinds:
            for f64 in dtypes:
                for batch, tiled in shapes:
                    yield name, key, value, kind, f64, batch, tiled


def point_id(name, key, value, kind, f64, batch, tiled):
    state = "default" if key is None else f"{key}={value}"
    return f"{name} {state} {kind} {'f64' if f64 else 'f32'} {batch} {'tiled' if tiled else 'soa'}"


def compute():
    """{point id: record}; the tuning is back at its defaults afterwards."""
    out = {}
    models = {}
    state = None
    try:
        for p in points():
            name, key, value = p[:3]
            if (key, value) != state:
                if state and state[0]:
                    ffi.set_tuning(state[0], -1)
                if key:
                    ffi.set_tuning(key, value)
                state = (key, value)
            mb = models.get(name) or models.setdefault(name, MODELS[name]())
            out[point_id(*p)] = record(mb.jit_source(p[4], p[3], batch=p[5], tiled=p[6]))
    finally:
        if state and state[0]:
            ffi.set_tuning(state[0], -1)
    return out


if __name__ == "__main__":
    data = compute()
    with open(OUT, "w") as f:
        json.dump(data, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, len(data), "points,", len({v["sha1"] for v in data.values()}), "distinct sources")
