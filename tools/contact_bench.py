"""The fused contact rollout (rollout_contact_batch) beside the composed per-step sequence of existing
entry points -- contact_wrench_batch, fd_ext_batch, two torch updates and the trajectory copy -- on
the same inputs: FR3 with 2 contact points and floating14 with 4, 65536 configurations, K = 16, fp32
and fp64, SoA rows.  The two candidates of a (model, dtype) are interleaved round by round in one
process; a round times `steps` calls between one hipEvent pair after a warm-up; the figures are the
median, minimum and every round.  The state is reset before every call (a copy outside the timed
region would not stay outside a stream's order, so it is inside, for both candidates alike).  Prints
one JSON object and writes it to --out.

--resources: no GPU.  Compiles the contact_wrench / rollout_contact kernels of FR3, the 16-link
chain, tree9 and floating14 (the point sets of tests/contact_ref.py) for gfx950 (hipRTC) and prints
registers, scratch and waves per SIMD from each code object's metadata (llvm-readelf --notes).

usage: python tools/contact_bench.py [--steps 20] [--rounds 5] [--out profiles/contact/contact_bench.json]
       python tools/contact_bench.py --resources [--out profiles/contact/resources.json]
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

DT, K = 1e-3, 16


def resources():
    """Registers / scratch / occupancy of every contact kernel, from RB_JIT_DUMP code objects."""
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        os.environ["RB_JIT_DUMP"] = d
        import contact_ref as cr

        for case in ("fr3", "chain16", "tree9", "floating14"):
            mb = cr.setup(case, 8, 91)[0]
            for rollout in (0, 1):
                for f64 in (1, 0):
                    before = set(os.listdir(d))
                    mb.contact_jit_compile(rollout, f64, "gfx950")
                    co = sorted(f for f in set(os.listdir(d)) - before if f.endswith(".co"))[-1]
                    notes = subprocess.run([readelf, "--notes", os.path.join(d, co)], capture_output=True, text=True).stdout

                    def field(name):
                        m = re.search(r"\.%s:\s+(\d+)" % name, notes)
                        return int(m.group(1)) if m else -1

                    vg = field("vgpr_count")  # gfx950 metadata: the unified count (arch + acc)
                    waves = min(8, 512 // max(8, -(-vg // 8) * 8))
                    out[f"{case}:{'rollout_contact' if rollout else 'contact_wrench'}:{'f64' if f64 else 'f32'}"] = {
                        "points": mb.n_contacts, "vgpr": vg, "agpr": field("agpr_count"), "sgpr": field("sgpr_count"),
                        "scratch_bytes": field("private_segment_fixed_size"),
                        "lds_bytes": field("group_segment_fixed_size"), "waves_per_simd": waves}
    return out


def _models():
    """(name, plain handle, handle with the set): FR3 with 2 points, floating14 with 4."""
    import ext_wrench_ref as xr

    fr3 = xr.setup("fr3")[0]
    fl = xr.setup("floating14")[0]
    par, _ = fl.topology()
    leaves = [j for j in range(fl.n) if j not in set(par)]
    sets = (("fr3", fr3, [fr3.n - 1, fr3.n - 1], [[0.05, 0.0, 0.1], [-0.05, 0.0, 0.1]], 0.4),
            ("floating14", fl, (leaves + leaves)[:4], [[0.0, 0.05, 0.1]] * 4, 0.0))
    for name, mb, links, points, offset in sets:
        yield name, mb, mb.with_contacts(links, points, offset=offset, stiffness=2000.0, damping=0.5, friction=0.7,
                                         slip_velocity=0.01)


def timings(a):
    import torch

    from rigidbody_amd import chains, ffi

    dev = torch.device("cuda:0")
    B = a.batch
    out = {"batch": B, "K": K, "dt": DT, "steps": a.steps, "rounds": a.rounds, "models": {}}
    for name, plain, mb in _models():
        n, lim = mb.n, mb.limits()
        res = {"n": n, "points": mb.n_contacts}
        for tname, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            x = {}
            for k, kind in enumerate(("q", "qd")):
                x[kind] = torch.empty((n, B), dtype=dtype, device=dev)
                ffi.fill_uniform(x[kind], *chains.input_ranges(lim, kind), chains.SEED + k)
            tau = torch.empty((K * n, B), dtype=dtype, device=dev)
            lo, hi = chains.input_ranges(lim, "tau")
            ffi.fill_uniform(tau, list(lo) * K, list(hi) * K, chains.SEED + 2)
            tau = tau.view(K, n, B)
            q, qd = torch.empty_like(x["q"]), torch.empty_like(x["qd"])
            traj = torch.empty_like(tau)
            fext = torch.empty((6 * n, B), dtype=dtype, device=dev)
            cforce = torch.empty((3 * mb.n_contacts, B), dtype=dtype, device=dev)
            acc = torch.empty_like(q)

            def fused():
                q.copy_(x["q"])
                qd.copy_(x["qd"])
                mb.rollout_contact_batch(q, qd, tau, DT, traj=traj)

            def composed():
                q.copy_(x["q"])
                qd.copy_(x["qd"])
                for k in range(K):
                    mb.contact_wrench_batch(q, qd, fext=fext, cforce=cforce)
                    plain.fd_ext_batch(q, qd, tau[k], fext, out=acc)
                    qd.add_(acc, alpha=DT)
                    q.add_(qd, alpha=DT)
                    traj[k].copy_(q)

            cands = {"fused": fused, "composed": composed}
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
            r["composed_over_fused"] = r["composed"]["us_median"] / r["fused"]["us_median"]
            res[tname] = r
        out["models"][name] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1 << 16)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = resources() if a.resources else timings(a)
    txt = json.dumps(out, indent=1)
    print(txt)
    dflt = os.path.join(REPO, "profiles", "contact", "resources.json" if a.resources else "contact_bench.json")
    path = a.out or dflt
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
