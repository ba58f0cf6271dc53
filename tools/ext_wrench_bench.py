"""rnea_ext_batch / fd_ext_batch against rnea_batch / fd_batch on the same inputs (FR3, 2^20
configurations, fp64 and fp32, SoA rows).  The four candidates of a dtype are interleaved round by
round in one process; each round times `steps` launches between one hipEvent pair after a spin-up
(bench.time_launches, as tools/deriv_bench.py); the figures are the median, minimum and every round.
Bytes per configuration: the plain kernels move 4 n values, the external-wrench ones 10 n (6 n
more rows of fext); hbm_frac is bytes / median time / the 8 TB/s peak.  Prints one JSON object and
writes it to --out.

--resources: no GPU.  Compiles the rnea_ext / fd_ext kernels of FR3, the 12-link general-axes
chain, the 30-link chain, tree9 and floating14 for gfx950 (hipRTC) and prints registers, scratch
and waves per SIMD from each code object's metadata (llvm-readelf --notes).

usage: python tools/ext_wrench_bench.py [--steps 20] [--rounds 5] [--out profiles/ext_wrench/ext_wrench_bench.json]
       python tools/ext_wrench_bench.py --resources
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


def resources():
    """Registers / scratch / occupancy of every external-wrench kernel, from RB_JIT_DUMP code objects."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        os.environ["RB_JIT_DUMP"] = d
        import ext_wrench_ref as xr

        for case in ("fr3", "general12", "chain30", "tree9", "floating14"):
            mb = xr.setup(case)[0]
            for fd in (0, 1):
                for f64 in (1, 0):
                    before = set(os.listdir(d))
                    mb.ext_jit_compile(fd, f64, "gfx950")
                    co = sorted(f for f in set(os.listdir(d)) - before if f.endswith(".co"))[-1]
                    notes = subprocess.run([readelf, "--notes", os.path.join(d, co)], capture_output=True, text=True).stdout

                    def field(name):
                        m = re.search(r"\.%s:\s+(\d+)" % name, notes)
                        return int(m.group(1)) if m else -1

                    vg, ag = field("vgpr_count"), field("agpr_count")
                    total = vg  # gfx950 metadata: vgpr_count is the unified count (arch + acc)
                    waves = min(8, 512 // max(8, -(-total // 8) * 8))
                    out[f"{case}:{'fd_ext' if fd else 'rnea_ext'}:{'f64' if f64 else 'f32'}"] = {
                        "vgpr": vg, "agpr": ag, "sgpr": field("sgpr_count"), "scratch_bytes": field("private_segment_fixed_size"),
                        "lds_bytes": field("group_segment_fixed_size"), "waves_per_simd": waves}
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ext_wrench", "ext_wrench_bench.json"))
    a = ap.parse_args()
    if a.resources:
        return resources()
    import torch

    import bench
    from rigidbody_amd import chains, ffi

    dev = torch.device("cuda:0")
    mb = ffi.Multibody.new()
    mb.upload()
    n, B = mb.n, a.batch
    lib, h, lim = ffi.lib(), mb.handle, mb.limits()
    out = {"model": "fr3", "n": n, "batch": B, "steps": a.steps, "rounds": a.rounds, "dtypes": {}}
    for name in ("f64", "f32"):
        dtype, es = bench.DT[name], 4 if name == "f32" else 8
        x = {}
        for k, kind in enumerate(("q", "qd", "qdd", "tau")):
            x[kind] = torch.empty((n, B), dtype=dtype, device=dev)
            ffi.fill_uniform(x[kind], *chains.input_ranges(lim, kind), chains.SEED + k)
        fext = torch.empty((6 * n, B), dtype=dtype, device=dev)
        amp = [20.0] * 3 + [5.0] * 3  # N, N m
        ffi.fill_uniform(fext, [-v for v in amp] * n, amp * n, chains.SEED + 9)
        o = torch.empty((n, B), dtype=dtype, device=dev)
        p = {k: v.data_ptr() for k, v in x.items()}
        fn = {k: getattr(lib, f"multibody_{k}_batch_{name}") for k in ("rnea", "fd", "rnea_ext", "fd_ext")}

        def plain(k, third):
            return lambda i, sp: fn[k](h, p["q"], p["qd"], p[third], o.data_ptr(), B, B, sp)

        def ext(k, third):
            return lambda i, sp: fn[k](h, p["q"], p["qd"], p[third], fext.data_ptr(), o.data_ptr(), B, B, sp)

        cands = {"rnea": plain("rnea", "qdd"), "rnea_ext": ext("rnea_ext", "qdd"), "fd": plain("fd", "tau"),
                 "fd_ext": ext("fd_ext", "tau")}
        sp0 = bench.ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for k, f in cands.items():
            assert f(0, sp0) == 0, (k, ffi.last_error())
        torch.cuda.synchronize()
        ms = {k: [] for k in cands}
        for r in range(a.rounds):
            for k, f in cands.items():
                _, t = bench.time_launches(f, a.steps, 2, 1, 50.0 if r == 0 else 10.0)
                ms[k].append(t)
        res = {}
        for k, v in ms.items():
            nbytes = (10 if k.endswith("_ext") else 4) * n * es * B
            med = float(np.median(v))
            res[k] = {"us_median": 1e3 * med, "us_min": 1e3 * float(np.min(v)), "us_rounds": [1e3 * float(t) for t in v],
                      "bytes_per_config": nbytes // B, "hbm_frac": nbytes / (med * 1e-3) / bench.HBM_PEAK}
        res["rnea_ext_over_rnea"] = res["rnea_ext"]["us_median"] / res["rnea"]["us_median"]
        res["fd_ext_over_fd"] = res["fd_ext"]["us_median"] / res["fd"]["us_median"]
        res["byte_ratio"] = 2.5
        out["dtypes"][name] = res
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
