"""The gradient of the fused contact rollout (rollout_contact_vjp_batch) beside the gradient of the
contact-free rollout on the plain handle (rollout_vjp_batch) and the forward contact rollout
(rollout_contact_batch): FR3 with contact_bench's 2 points, 65536 configurations, K = 16, fp32 and
fp64, SoA rows, one process.  The method is contact_bench.py's: the candidates of a dtype are
interleaved round by round; a round times `steps` calls between one hipEvent pair after a warm-up;
median, minimum and every round are kept.  The forward rollout resets its state inside the timed
region (as there); the gradients do not modify theirs.  Prints one JSON object and writes it to --out.

--resources: no GPU.  Compiles the rollout_contact_vjp kernel of FR3, the 12-link chain and the
general-axis 7-link chain (the point sets of tests/contact_ref.py), and FR3's rollout_vjp kernel beside
it, for gfx950 (hipRTC) and prints registers, scratch and waves per SIMD from each code object.

usage: python tools/contact_vjp_bench.py [--steps 10] [--rounds 5] [--out profiles/contact_vjp/contact_vjp_bench.json]
       python tools/contact_vjp_bench.py --resources [--out profiles/contact_vjp/resources.json]
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
sys.path[:0] = [REPO, os.path.join(REPO, "rigidbody-rs_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]

DT, K = 1e-3, 16


def resources():
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        os.environ["RB_JIT_DUMP"] = d
        import contact_ref as cr

        for case in ("fr3", "chain12", "general7"):
            mb, plain = cr.setup(case, 8, 91)[:2]
            kinds = [("rollout_contact_vjp", mb.contact_vjp_jit_compile)]
            if case == "fr3":
                kinds.append(("rollout_vjp", plain.rollout_vjp_jit_compile))
            for kname, compile_ in kinds:
                for f64 in (1, 0):
                    before = set(os.listdir(d))
                    compile_(f64, "gfx950")
                    co = sorted(f for f in set(os.listdir(d)) - before if f.endswith(".co"))[-1]
                    notes = subprocess.run([readelf, "--notes", os.path.join(d, co)], capture_output=True, text=True).stdout

                    def field(name):
                        m = re.search(r"\.%s:\s+(\d+)" % name, notes)
                        return int(m.group(1)) if m else -1

                    vg = field("vgpr_count")  # gfx950 metadata: the unified count (arch + acc)
                    out[f"{case}:{kname}:{'f64' if f64 else 'f32'}"] = {
                        "points": mb.n_contacts, "vgpr": vg, "agpr": field("agpr_count"), "sgpr": field("sgpr_count"),
                        "scratch_bytes": field("private_segment_fixed_size"),
                        "lds_bytes": field("group_segment_fixed_size"),
                        "waves_per_simd": min(8, 512 // max(8, -(-vg // 8) * 8))}
    return out


def timings(a):
    import torch

    from contact_bench import _models
    from rigidbody_amd import chains, ffi

    dev = torch.device("cuda:0")
    B = a.batch
    name, plain, mb = next(_models())  # FR3, 2 points
    n, lim = mb.n, mb.limits()
    out = {"batch": B, "K": K, "dt": DT, "steps": a.steps, "rounds": a.rounds, "model": name, "n": n,
           "points": mb.n_contacts}
    for tname, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        x = {}
        for k, kind in enumerate(("q", "qd")):
            x[kind] = torch.empty((n, B), dtype=dtype, device=dev)
            ffi.fill_uniform(x[kind], *chains.input_ranges(lim, kind), chains.SEED + k)
        tau = torch.empty((K * n, B), dtype=dtype, device=dev)
        lo, hi = chains.input_ranges(lim, "tau")
        ffi.fill_uniform(tau, list(lo) * K, list(hi) * K, chains.SEED + 2)
        tau = tau.view(K, n, B)
        gq, gqd = torch.randn_like(tau), torch.randn_like(tau)
        q, qd, traj = torch.empty_like(x["q"]), torch.empty_like(x["qd"]), torch.empty_like(tau)

        def forward():
            q.copy_(x["q"])
            qd.copy_(x["qd"])
            mb.rollout_contact_batch(q, qd, tau, DT, traj=traj)

        cands = {"rollout_contact_vjp": lambda: mb.rollout_contact_vjp_batch(x["q"], x["qd"], tau, DT, gq, gqd),
                 "rollout_vjp": lambda: plain.rollout_vjp_batch(x["q"], x["qd"], tau, DT, gq, gqd),
                 "rollout_contact": forward}
        for f in cands.values():  # compile, warm up
            f()
        torch.cuda.synchronize()
        ms = {k: [] for k in cands}
        for _ in range(a.rounds):
            for k, f in cands.items():
                f()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    f()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1) / a.steps)
        r = {k: {"us_median": 1e3 * float(np.median(v)), "us_min": 1e3 * float(np.min(v)),
                 "us_rounds": [1e3 * float(t) for t in v]} for k, v in ms.items()}
        v = r["rollout_contact_vjp"]["us_median"]
        r["vjp_over_plain_vjp"] = v / r["rollout_vjp"]["us_median"]
        # the only correct alternative before this kernel: central differences over rollout_contact,
        # 2 launches per input element, n (K + 2) elements
        r["central_differences_launches"] = 2 * n * (K + 2)
        r["central_differences_over_vjp"] = 2 * n * (K + 2) * r["rollout_contact"]["us_median"] / v
        out[tname] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1 << 16)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = resources() if a.resources else timings(a)
    txt = json.dumps(out, indent=1)
    print(txt)
    dflt = os.path.join(REPO, "profiles", "contact_vjp", "resources.json" if a.resources else "contact_vjp_bench.json")
    path = a.out or dflt
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
