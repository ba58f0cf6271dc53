"""fd_vjp_batch (wrench form) and fd_vjp_plain_batch beside their neighbours on the same inputs: a plain
fd_ext_batch launch (the forward it differentiates and repeats), an rnea_vjp_batch launch (its second
stage alone) and -- FR3 only -- the composition a caller had to write before: fd_ext_batch, crba_batch, the
symmetrised mass matrix and torch.linalg.solve for mu, rnea_vjp_batch at (q, qd, qdd, mu), three negations.
FR3 and the floating-base tree, fp64 and fp32, 2^20 and 2^16 configurations, SoA rows.  The candidates of a
group are interleaved round by round in one process; each round replays a captured HIP graph of
`per_graph` launches between one hipEvent pair after a spin-up (bench.time_graph); the figures are the
median, minimum and every round.  The composition alone is timed eagerly between events (torch.linalg.solve
cannot be captured), after the others.  Algorithmic values per configuration: fd_vjp 4 n + 6 n in, 4 n + 6 n out;
fd_vjp_plain 4 n + 4 n; fd_ext 3 n + 6 n + n; rnea_vjp 4 n + 6 n + 3 n + 6 n; hbm_frac is bytes / median time
/ the 8 TB/s peak (not given for the composition, whose traffic is mostly torch's).  Prints one JSON object
and writes it to --out.

--resources: no GPU.  Compiles both kernels of FR3, the 30-link chain, tree9 and floating14 for gfx950
(hipRTC) and prints registers, scratch, LDS and waves per SIMD from each code object's metadata
(llvm-readelf --notes).

usage: python tools/fd_vjp_bench.py [--steps 200] [--rounds 5] [--out profiles/fd_vjp/fd_vjp_bench.json]
       python tools/fd_vjp_bench.py --resources [--out profiles/fd_vjp/resources.json]
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

VARIANTS = ("plain", "wrench")


def resources():
    """Registers / scratch / occupancy of both fd_vjp kernels, from RB_JIT_DUMP code objects."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        os.environ["RB_JIT_DUMP"] = d
        import ext_wrench_ref as xr

        for case in ("fr3", "chain30", "tree9", "floating14"):
            mb = xr.setup(case)[0]
            for ext, variant in enumerate(VARIANTS):
                for f64 in (1, 0):
                    before = set(os.listdir(d))
                    mb.fd_vjp_jit_compile(ext, f64, "gfx950")
                    co = sorted(f for f in set(os.listdir(d)) - before if f.endswith(".co"))[-1]
                    notes = subprocess.run([readelf, "--notes", os.path.join(d, co)], capture_output=True, text=True).stdout

                    def field(name):
                        m = re.search(r"\.%s:\s+(\d+)" % name, notes)
                        return int(m.group(1)) if m else -1

                    vg = field("vgpr_count")  # gfx950 metadata: the unified count (arch + acc)
                    waves = min(8, 512 // max(8, -(-vg // 8) * 8))
                    out[f"{case}:{variant}:{'f64' if f64 else 'f32'}"] = {
                        "vgpr": vg, "agpr": field("agpr_count"), "sgpr": field("sgpr_count"),
                        "scratch_bytes": field("private_segment_fixed_size"),
                        "lds_bytes": field("group_segment_fixed_size"), "waves_per_simd": waves}
    return out


def timings(a):
    import torch

    import bench
    import ext_wrench_ref as xr
    from rigidbody_amd import chains, ffi

    dev = torch.device("cuda:0")
    lib = ffi.lib()
    out = {"steps": a.steps, "per_graph": a.per_graph, "rounds": a.rounds, "groups": {}}
    for case in ("fr3", "floating14"):
        mb = xr.setup(case)[0]
        mb.upload()
        n, h, lim = mb.n, mb.handle, mb.limits()
        for name in ("f64", "f32"):
            dtype, es = bench.DT[name], 4 if name == "f32" else 8
            for B in a.batches:
                x = {}
                for k, kind in enumerate(("q", "qd", "tau")):
                    x[kind] = torch.empty((n, B), dtype=dtype, device=dev)
                    ffi.fill_uniform(x[kind], *chains.input_ranges(lim, kind), chains.SEED + k)
                amp = np.tile([xr.FORCE] * 3 + [xr.MOMENT] * 3, n)
                x["fext"] = torch.empty((6 * n, B), dtype=dtype, device=dev)
                ffi.fill_uniform(x["fext"], -amp, amp, chains.SEED + 3)
                x["w"] = torch.empty((n, B), dtype=dtype, device=dev)
                ffi.fill_uniform(x["w"], -np.ones(n), np.ones(n), chains.SEED + 4)
                g = [torch.empty((n, B), dtype=dtype, device=dev) for _ in range(4)]  # qdd, g_q, g_qd, g_tau
                gf = torch.empty((6 * n, B), dtype=dtype, device=dev)
                p = {k: v.data_ptr() for k, v in x.items()}
                gp = [t.data_ptr() for t in g]
                vjp = getattr(lib, f"multibody_fd_vjp_batch_{name}")
                plain = getattr(lib, f"multibody_fd_vjp_plain_batch_{name}")
                fdx = getattr(lib, f"multibody_fd_ext_batch_{name}")
                rvjp = getattr(lib, f"multibody_rnea_vjp_batch_{name}")
                cands = {
                    "fd_vjp": (lambda i, sp: vjp(h, p["q"], p["qd"], p["tau"], p["fext"], p["w"], *gp, gf.data_ptr(), B, B,
                                                 sp), 20 * n),
                    "fd_vjp_plain": (lambda i, sp: plain(h, p["q"], p["qd"], p["tau"], p["w"], *gp, B, B, sp), 8 * n),
                    "fd_ext": (lambda i, sp: fdx(h, p["q"], p["qd"], p["tau"], p["fext"], gp[0], B, B, sp), 10 * n),
                    # (qdd's place takes tau: any finite rows time the same)
                    "rnea_vjp": (lambda i, sp: rvjp(h, p["q"], p["qd"], p["tau"], p["fext"], p["w"], gp[1], gp[2], gp[3],
                                                    gf.data_ptr(), B, B, sp), 19 * n),
                }
                if case == "fr3":  # the composition INTEGRATION.md used to describe
                    crba = getattr(lib, f"multibody_crba_batch_{name}")
                    Hm = torch.empty((n * n, B), dtype=dtype, device=dev)
                    Hs = torch.empty((B, n, n), dtype=dtype, device=dev)
                    mu = torch.empty((n, B), dtype=dtype, device=dev)
                    scratch = torch.empty((n, B), dtype=dtype, device=dev)

                    def composition(i, sp):
                        rc = fdx(h, p["q"], p["qd"], p["tau"], p["fext"], gp[0], B, B, sp)
                        rc |= crba(h, p["q"], Hm.data_ptr(), B, B, sp)
                        U = torch.triu(Hm.view(n, n, B).permute(2, 1, 0))  # [b, row, col], the ABI's upper triangle
                        torch.add(U, torch.triu(U, 1).transpose(1, 2), out=Hs)
                        mu.copy_(torch.linalg.solve(Hs, x["w"].t().unsqueeze(-1)).squeeze(-1).t())
                        rc |= rvjp(h, p["q"], p["qd"], gp[0], p["fext"], mu.data_ptr(), gp[1], gp[2], scratch.data_ptr(),
                                   gf.data_ptr(), B, B, sp)
                        for t in (g[1], g[2], gf):
                            t.neg_()
                        return rc

                else:
                    composition = None
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
                    med = float(np.median(v))
                    res[k] = {"us_median": 1e3 * med, "us_min": 1e3 * float(np.min(v)),
                              "us_rounds": [1e3 * float(t) for t in v]}
                    if cands[k][1] is not None:
                        nbytes = cands[k][1] * es * B
                        res[k].update(bytes_per_config=nbytes // B, hbm_frac=nbytes / (med * 1e-3) / bench.HBM_PEAK)
                if composition is not None:
                    # torch.linalg.solve allocates and checks its result on the host, so it cannot be captured:
                    # timed eagerly, `steps` calls between one event pair per round (launch overhead included)
                    v = []
                    for r in range(a.rounds):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        assert composition(0, sp0) == 0
                        e0.record()
                        for _ in range(max(1, a.steps // 10)):
                            composition(0, sp0)
                        e1.record()
                        torch.cuda.synchronize()
                        v.append(e0.elapsed_time(e1) / max(1, a.steps // 10))
                    res["fd_ext_crba_solve_rnea_vjp"] = {"us_median": 1e3 * float(np.median(v)), "us_min": 1e3 * float(np.min(v)),
                                                         "us_rounds": [1e3 * float(t) for t in v], "timed": "eager, events"}
                out["groups"][f"{case}:{name}:{B}"] = res
                print(f"{case}:{name}:{B} measured", file=sys.stderr, flush=True)
                del x, g, gf
                torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--per-graph", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[1 << 20, 1 << 16])
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = resources() if a.resources else timings(a)
    txt = json.dumps(out, indent=1)
    print(txt)
    dflt = os.path.join(REPO, "profiles", "fd_vjp", "resources.json" if a.resources else "fd_vjp_bench.json")
    path = a.out or dflt
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
