"""com_batch / centroidal_batch / cmm_batch beside link_vel_batch, the sweep they share, on the same
inputs (FR3, 2^20 configurations, fp64 and fp32, SoA rows).  The four candidates of a dtype are
interleaved round by round in one process; each round replays a captured HIP graph of `per_graph`
launches between one hipEvent pair after a spin-up (bench.time_graph); the figures are the median,
minimum and every round.  Algorithmic bytes per configuration: com (n + 3) values, centroidal
(2 n + 11), cmm (n + 6 n), link_vel (2 n + 6 n); hbm_frac is bytes / median time / the 8 TB/s peak.
Prints one JSON object and writes it to --out.

--resources: no GPU.  Compiles the three kernels of FR3, the 30-link chain, tree9 and floating14 for
gfx950 (hipRTC) and prints registers, scratch, LDS and waves per SIMD from each code object's
metadata (llvm-readelf --notes).

usage: python tools/centroidal_bench.py [--steps 200] [--rounds 5] [--out profiles/centroidal/centroidal_bench.json]
       python tools/centroidal_bench.py --resources [--out profiles/centroidal/resources.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "rigidbody-rs_amd"), os.path.join(REPO, "tests")]

KERNELS = ("com", "centroidal", "cmm")


def resources():
    """Registers / scratch / occupancy of every centroidal kernel, from RB_JIT_DUMP code objects."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        os.environ["RB_JIT_DUMP"] = d
        import ext_wrench_ref as xr

        for case in ("fr3", "chain30", "tree9", "floating14"):
            mb = xr.setup(case)[0]
            for which, kernel in enumerate(KERNELS):
                for f64 in (1, 0):
                    before = set(os.listdir(d))
                    mb.centroidal_jit_compile(which, f64, "gfx950")
                    co = sorted(f for f in set(os.listdir(d)) - before if f.endswith(".co"))[-1]
                    notes = subprocess.run([readelf, "--notes", os.path.join(d, co)], capture_output=True, text=True).stdout

                    def field(name):
                        m = re.search(r"\.%s:\s+(\d+)" % name, notes)
                        return int(m.group(1)) if m else -1

                    vg = field("vgpr_count")  # gfx950 metadata: the unified count (arch + acc)
                    waves = min(8, 512 // max(8, -(-vg // 8) * 8))
                    out[f"{case}:{kernel}:{'f64' if f64 else 'f32'}"] = {
                        "vgpr": vg, "agpr": field("agpr_count"), "sgpr": field("sgpr_count"),
                        "scratch_bytes": field("private_segment_fixed_size"),
                        "lds_bytes": field("group_segment_fixed_size"), "waves_per_simd": waves}
    return out


def timings(a):
    import torch

    import bench
    from rigidbody_amd import chains, ffi

    dev = torch.device("cuda:0")
    mb = ffi.Multibody.new()
    mb.upload()
    n, B = mb.n, a.batch
    lib, h, lim = ffi.lib(), mb.handle, mb.limits()
    out = {"model": "fr3", "n": n, "batch": B, "steps": a.steps, "per_graph": a.per_graph, "rounds": a.rounds,
           "dtypes": {}}
    for name in ("f64", "f32"):
        dtype, es = bench.DT[name], 4 if name == "f32" else 8
        x = {}
        for k, kind in enumerate(("q", "qd")):
            x[kind] = torch.empty((n, B), dtype=dtype, device=dev)
            ffi.fill_uniform(x[kind], *chains.input_ranges(lim, kind), chains.SEED + k)
        com, hg, en, ag, vel = (torch.empty((r, B), dtype=dtype, device=dev) for r in (3, 6, 2, 6 * n, 6 * n))
        q, qd = x["q"].data_ptr(), x["qd"].data_ptr()
        fn = {k: getattr(lib, f"multibody_{k}_batch_{name}") for k in KERNELS + ("link_vel",)}
        cands = {"com": (lambda i, sp: fn["com"](h, q, com.data_ptr(), B, B, sp), n + 3),
                 "centroidal": (lambda i, sp: fn["centroidal"](h, q, qd, com.data_ptr(), hg.data_ptr(), en.data_ptr(),
                                                               B, B, sp), 2 * n + 11),
                 "cmm": (lambda i, sp: fn["cmm"](h, q, ag.data_ptr(), B, B, sp), 7 * n),
                 "link_vel": (lambda i, sp: fn["link_vel"](h, q, qd, vel.data_ptr(), B, B, sp), 8 * n)}
        sp0 = bench.ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for k, (f, _) in cands.items():
            assert f(0, sp0) == 0, (k, ffi.last_error())
        torch.cuda.synchronize()
        ms = {k: [] for k in cands}
        for r in range(a.rounds):
            for k, (f, _) in cands.items():
                _, t, _ = bench.time_graph(f, a.steps, a.per_graph, 100.0 if r == 0 else 20.0)
                ms[k].append(t)
        res = {}
        for k, v in ms.items():
            nbytes = cands[k][1] * es * B
            med = float(np.median(v))
            res[k] = {"us_median": 1e3 * med, "us_min": 1e3 * float(np.min(v)), "us_rounds": [1e3 * float(t) for t in v],
                      "bytes_per_config": nbytes // B, "hbm_frac": nbytes / (med * 1e-3) / bench.HBM_PEAK}
        out["dtypes"][name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--per-graph", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = resources() if a.resources else timings(a)
    txt = json.dumps(out, indent=1)
    print(txt)
    dflt = os.path.join(REPO, "profiles", "centroidal", "resources.json" if a.resources else "centroidal_bench.json")
    path = a.out or dflt
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
