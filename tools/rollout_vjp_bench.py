"""One rollout_vjp_batch launch against the composition a caller had before it existed: K
fd_deriv_batch launches (qdd and the three Jacobians of every step, kept for the backward sweep),
the semi-implicit Euler step in torch, then the adjoint recursion as batched matrix-vector products
in torch (an elementwise product and a reduction over the SoA matrices: one pass over each).

FR3, K = 16, 65536 configurations fp32 and 2^20 fp64.  The two candidates are interleaved round by
round in one process; each round times `steps` repetitions between one hipEvent pair after a
spin-up, as tools/deriv_bench.py does; the figures are the median, minimum and every round.  Both
compute the same gradient (checked once per shape before timing).  Prints one JSON object and writes
it to --out.

usage: python tools/rollout_vjp_bench.py [--steps 5] [--rounds 5] [--out profiles/rollout_vjp/rollout_vjp_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "rigidbody-rs_amd")]
import bench  # noqa: E402
from rigidbody_amd import chains, ffi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--K", type=int, default=16)
    ap.add_argument("--shapes", nargs="+", default=["f32:65536", "f64:1048576"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rollout_vjp", "rollout_vjp_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    mb = ffi.Multibody.new()
    mb.upload()
    n, K, dt = mb.n, a.K, 0.01
    lib, h, lim = ffi.lib(), mb.handle, mb.limits()
    out = {"model": "fr3", "n": n, "K": K, "dt": dt, "steps": a.steps, "rounds": a.rounds, "shapes": {}}
    for shape in a.shapes:
        name, B = shape.split(":")
        B = int(B)
        dtype, es = bench.DT[name], 4 if name == "f32" else 8
        q, qd = (torch.empty((n, B), dtype=dtype, device=dev) for _ in range(2))
        ffi.fill_uniform(q, *chains.input_ranges(lim, "q"), chains.SEED)
        ffi.fill_uniform(qd, *chains.input_ranges(lim, "qd"), chains.SEED + 1)
        # torques of moderate accelerations, tau_k = rnea(q, qd, qdd_k), qdd_k ~ U(-3, 3): torques drawn
        # over the effort limits drive the 16-step trajectory out of the input domain
        tau = torch.empty((K, n, B), dtype=dtype, device=dev)
        qdd = torch.empty((n, B), dtype=dtype, device=dev)
        for k in range(K):
            ffi.fill_uniform(qdd, [-3.0] * n, [3.0] * n, chains.SEED + 2 + k)
            mb.rnea_batch(q, qd, qdd, out=tau[k])
        gq, gqd = torch.randn_like(tau), torch.randn_like(tau)
        g = [torch.empty_like(q), torch.empty_like(q), torch.empty_like(tau)]
        work = torch.empty((K, 2 * n, B), dtype=dtype, device=dev)
        f_vjp = getattr(lib, f"multibody_rollout_vjp_batch_{name}")
        f_fd = getattr(lib, f"multibody_fd_deriv_batch_{name}")
        # the composition's own storage: every step's state, acceleration and three matrices
        qs, vs = torch.empty_like(work[:, :n]), torch.empty_like(work[:, :n])
        acc = torch.empty((n, B), dtype=dtype, device=dev)
        mats = torch.empty((K, 3, n * n, B), dtype=dtype, device=dev)
        c = [torch.empty_like(q), torch.empty_like(q), torch.empty_like(tau)]

        def vjp(i, sp):
            assert f_vjp(h, q.data_ptr(), qd.data_ptr(), tau.data_ptr(), dt, K, gq.data_ptr(), gqd.data_ptr(),
                         *[t.data_ptr() for t in g], work.data_ptr(), B, B, sp) == 0

        def tmul(m, x):  # M^T x per configuration; m [n*n, B] with row i + n k = M[i, k]
            return (m.view(n, n, B) * x.unsqueeze(0)).sum(1)

        def composed(i, sp):
            qk, vk = q, qd
            for k in range(K):
                qs[k].copy_(qk)
                vs[k].copy_(vk)
                assert f_fd(h, qs[k].data_ptr(), vs[k].data_ptr(), tau[k].data_ptr(), acc.data_ptr(),
                            *[mats[k, j].data_ptr() for j in range(3)], B, B, sp) == 0
                vk = vs[k] + dt * acc
                qk = qs[k] + dt * vk
            lq, lv = torch.zeros_like(q), torch.zeros_like(q)
            for k in reversed(range(K)):
                lq = lq + gq[k]
                vb = lv + gqd[k] + dt * lq
                ab = dt * vb
                c[2][k] = tmul(mats[k, 2], ab)
                lq = lq + tmul(mats[k, 0], ab)
                lv = vb + tmul(mats[k, 1], ab)
            c[0].copy_(lq)
            c[1].copy_(lv)

        sp0 = bench.ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        vjp(0, sp0)
        composed(0, sp0)
        torch.cuda.synchronize()
        agree = max(float(((x - y).abs().max() / (1 + y.abs().max()))) for x, y in zip(g, c))
        cands = {"rollout_vjp": vjp, "composition": composed}
        ms = {k: [] for k in cands}
        for r in range(a.rounds):
            for k, fn in cands.items():
                _, t = bench.time_launches(fn, a.steps, 2, 1, 50.0 if r == 0 else 10.0)
                ms[k].append(t)
        res = {k: {"us_median": 1e3 * float(np.median(v)), "us_min": 1e3 * float(np.min(v)),
                   "us_rounds": [1e3 * float(x) for x in v]} for k, v in ms.items()}
        res["agreement_scaled"] = agree
        res["speedup_vs_composition"] = res["composition"]["us_median"] / res["rollout_vjp"]["us_median"]
        # inputs + outputs + the workspace written and read once
        res["rollout_vjp"]["bytes_per_config"] = (4 * n + 4 * K * n + 2 * 2 * (K - 1) * n) * es
        out["shapes"][shape] = res
        del mats, work, tau, gq, gqd, qs, vs
        torch.cuda.empty_cache()
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
