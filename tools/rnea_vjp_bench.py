"""rnea_vjp_batch (wrench form) and rnea_vjp_plain_batch beside the two things a launch replaces, on the
same inputs: a plain rnea_ext_batch launch (the forward it differentiates), and -- FR3 only, the scope of
rnea_deriv -- rnea_deriv_batch plus the two matrix-vector products g_q = dtau_dq^T w, g_qd = dtau_dqd^T w
in torch (one broadcast multiply and one sum over i each, into preallocated tensors).  FR3 and the
floating-base tree, fp64 and fp32, 2^20 and 2^16 configurations, SoA rows.  The candidates of a group are
interleaved round by round in one process; each round replays a captured HIP graph of `per_graph`
launches between one hipEvent pair after a spin-up (bench.time_graph); the figures are the median,
minimum and every round.  Algorithmic values per configuration: rnea_vjp 4 n + 6 n in, 3 n + 6 n out;
rnea_vjp_plain 4 n + 3 n; rnea_ext 3 n + 6 n + n; hbm_frac is bytes / median time / the 8 TB/s peak (not
given for the composite, whose traffic is torch's).  Prints one JSON object and writes it to --out.

--resources: no GPU.  Compiles both kernels of FR3, the 30-link chain, tree9 and floating14 for gfx950
(hipRTC) and prints registers, scratch, LDS and waves per SIMD from each code object's metadata
(llvm-readelf --notes).

usage: python tools/rnea_vjp_bench.py [--steps 200] [--rounds 5] [--out profiles/rnea_vjp/rnea_vjp_bench.json]
       python tools/rnea_vjp_bench.py --resources [--out profiles/rnea_vjp/resources.json]
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
    """Registers / scratch / occupancy of both rnea_vjp kernels, from RB_JIT_DUMP code objects."""
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
                    mb.rnea_vjp_jit_compile(ext, f64, "gfx950")
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
                for k, kind in enumerate(("q", "qd", "qdd")):
                    x[kind] = torch.empty((n, B), dtype=dtype, device=dev)
                    ffi.fill_uniform(x[kind], *chains.input_ranges(lim, kind), chains.SEED + k)
                amp = np.tile([xr.FORCE] * 3 + [xr.MOMENT] * 3, n)
                x["fext"] = torch.empty((6 * n, B), dtype=dtype, device=dev)
                ffi.fill_uniform(x["fext"], -amp, amp, chains.SEED + 3)
                x["w"] = torch.empty((n, B), dtype=dtype, device=dev)
                ffi.fill_uniform(x["w"], -np.ones(n), np.ones(n), chains.SEED + 4)
                g = [torch.empty((n, B), dtype=dtype, device=dev) for _ in range(3)]
                gf = torch.empty((6 * n, B), dtype=dtype, device=dev)
                tau = torch.empty((n, B), dtype=dtype, device=dev)
                p = {k: v.data_ptr() for k, v in x.items()}
                gp = [t.data_ptr() for t in g]
                vjp = getattr(lib, f"multibody_rnea_vjp_batch_{name}")
                plain = getattr(lib, f"multibody_rnea_vjp_plain_batch_{name}")
                ext = getattr(lib, f"multibody_rnea_ext_batch_{name}")
                cands = {
                    "rnea_vjp": (lambda i, sp: vjp(h, p["q"], p["qd"], p["qdd"], p["fext"], p["w"], *gp, gf.data_ptr(),
                                                   B, B, sp), 19 * n),
                    "rnea_vjp_plain": (lambda i, sp: plain(h, p["q"], p["qd"], p["qdd"], p["w"], *gp, B, B, sp), 7 * n),
                    "rnea_ext": (lambda i, sp: ext(h, p["q"], p["qd"], p["qdd"], p["fext"], tau.data_ptr(), B, B, sp),
                                 10 * n),
                }
                if case == "fr3":  # rnea_deriv's scope: serial revolute chains
                    deriv = getattr(lib, f"multibody_rnea_deriv_batch_{name}")
                    dq, dqd, tmp = (torch.empty((n * n, B), dtype=dtype, device=dev) for _ in range(3))
                    w3 = x["w"].unsqueeze(0)  # row i + n k of dq is d tau_i / d q_k: view [k, i, b]

                    def composite(i, sp):
                        rc = deriv(h, p["q"], p["qd"], p["qdd"], dq.data_ptr(), dqd.data_ptr(), B, B, sp)
                        for m, o in ((dq, g[0]), (dqd, g[1])):
                            torch.mul(m.view(n, n, B), w3, out=tmp.view(n, n, B))
                            torch.sum(tmp.view(n, n, B), dim=1, out=o)
                        return rc

                    cands["rnea_deriv_plus_2_matvec"] = (composite, None)
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
                out["groups"][f"{case}:{name}:{B}"] = res
                print(f"{case}:{name}:{B} measured", file=sys.stderr, flush=True)
                del x, g, gf, tau
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
    dflt = os.path.join(REPO, "profiles", "rnea_vjp", "resources.json" if a.resources else "rnea_vjp_bench.json")
    path = a.out or dflt
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
