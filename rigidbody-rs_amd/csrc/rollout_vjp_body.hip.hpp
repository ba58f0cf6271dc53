// rollout_vjp_body.hip.hpp -- per-lane reverse-mode gradient (vector-Jacobian product) of the fused
// rollout of serial revolute chains on the mass-matrix forward dynamics (host + device).
//
// The rollout (aba_body.hip.hpp rollout_lane) steps, for k = 0 .. K-1,
//     a_k = fd(q_k, v_k, tau_k)     v_{k+1} = v_k + dt a_k     q_{k+1} = q_k + dt v_{k+1}
// Given cotangents gq[k], gqd[k] of the state after step k (gq[k] pairs with traj[k]), the adjoint
// sweep starts from lq = lv = 0 and runs k = K-1 .. 0:
//     lq += gq[k];  lv += gqd[k]
//     vb  = lv + dt lq                       (cotangent of v_{k+1})
//     mu  = sym(H(q_k))^-1 (dt vb)           -> g_tau[k] = mu      (d a / d tau = sym(H)^-1)
//     lq  = lq - (d rnea / d q )^T(q_k, v_k, a_k) mu               (d a / d q  = -sym(H)^-1 d rnea / d q)
//     lv  = vb - (d rnea / d qd)^T(q_k, v_k, a_k) mu
// and leaves g_q0 = lq, g_qd0 = lv.  Element c of (d rnea / d q)^T mu is the dot product of tangent
// column c with mu: rnea_deriv_core (rnea_deriv_body.hip.hpp) hands every column to a sink as it
// completes, so no n^2 value is stored or kept live, and the output is the size of the input.
//
// One configuration per lane, one launch.  Forward pass: steps 0 .. K-2 by fdh_eval's own stages and
// rollout_lane's fmadd order, the pre-step state (q_k, v_k) written to the caller's workspace
// work [K][2n][ld] (row 2n k + j: q_k[j], row 2n k + n + j: v_k[j]); a lane reads back only rows it
// wrote itself.  The state before the last step stays in registers (its row of `work` is not
// used), and that step's acceleration is the backward pass's own.  Backward pass per step: reload
// (q_k, v_k), bias + H + L D L^T + the solve for a_k, a second solve on the kept factors for mu, then
// the column sweeps with the two dot-product sinks.  State and the two adjoint vectors are held in
// registers between steps.
//
// Input domain.  q_k, v_k and tau_k are checked at every step (InputGuard, as the rollout) into one
// running check; it is complete -- every step seen -- before the backward pass stores anything, so a
// configuration whose q, qd or tau_seq leaves the domain at any step gets NaN in EVERY element of
// g_q0, g_qd0 and g_tau.  The cotangents gq, gqd are not checked: a NaN there propagates by
// arithmetic into the outputs it reaches.
#pragma once

#include "rnea_deriv_body.hip.hpp"

namespace rbamd {
namespace dev {

// bias, H = L D L^T and a = fd(q, v, tau) of one step, by fdh_eval's stages on the running check.
template <typename T, int N, bool FAST, typename Tau>
RB_HD void vjp_step_fd(const T *mdl, const T (&qv)[N], const T (&qdv)[N], Tau &&load_tau, T (&cs)[N], T (&sn)[N],
                       T (&H)[N][N], T (&Di)[N], T (&av)[N], InputGuard<T> &gd) {
    T C[N], tv[N];
    fdh_bias<T, N, FAST>(mdl, qv, qdv, cs, sn, C, gd);
    load_tau(tv);
    fdh_factor<T, N>(mdl, cs, sn, H, Di);
    gd.vals(tv);
    fdh_solve<T, N>(H, Di, tv, C, [&](int j, T v) { av[j] = v; });
}

// The two sweeps over a step of the caller's: step(k, qv, qdv, cs, sn, H, Di, av, gd) leaves step k's
// (cos, sin), the factors of H and a_k, every input of the step through gd; extra(qv, qdv, cs, sn, mu,
// lq, lv), after the column sweeps, adds what the step's generalised force has beyond rnea (the
// contact terms of contact_vjp_body.hip.hpp; nothing here).
// qv, qdv: the initial state (overwritten).  load_g(k, gq, gqd): step k's rows;
// work_st(k, r, v) / work_ld(k, r): row r < 2 N of step k's workspace; out_tau(k, j, v);
// out_state(j, g_q0_j, g_qd0_j).  K >= 1.
template <typename T, int N, typename Step, typename Extra, typename LoadG, typename WorkSt, typename WorkLd,
          typename OutTau, typename OutState>
RB_HD void rollout_adjoint_eval(const T *mdl, T (&qv)[N], T (&qdv)[N], T dt, int K, Step &&step, Extra &&extra,
                                LoadG &&load_g, WorkSt &&work_st, WorkLd &&work_ld, OutTau &&out_tau,
                                OutState &&out_state) {
    InputGuard<T> gd;
    for (int k = 0; k + 1 < K; ++k) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            work_st(k, j, qv[j]);
            work_st(k, N + j, qdv[j]);
        }
        T cs[N], sn[N], H[N][N], Di[N], av[N];
        step(k, qv, qdv, cs, sn, H, Di, av, gd);
#pragma unroll
        for (int j = 0; j < N; ++j) {
            qdv[j] = fmadd(dt, av[j], qdv[j]);
            qv[j] = fmadd(dt, qdv[j], qv[j]);
        }
    }
    T lq[N], lv[N], zero[N];
#pragma unroll
    for (int j = 0; j < N; ++j) lq[j] = lv[j] = zero[j] = T(0);
    for (int k = K - 1; k >= 0; --k) {
        if (k != K - 1) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                qv[j] = work_ld(k, j);
                qdv[j] = work_ld(k, N + j);
            }
        }
        // (the reloaded state passes the check a second time: the same values, the same verdict)
        T cs[N], sn[N], H[N][N], Di[N], av[N], vb[N], ab[N], mu[N];
        step(k, qv, qdv, cs, sn, H, Di, av, gd);
        {
            T gq[N], gqd[N];
            load_g(k, gq, gqd);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                lq[j] += gq[j];
                vb[j] = fmadd(dt, lq[j], lv[j] + gqd[j]);
                ab[j] = dt * vb[j];
            }
        }
        fdh_solve<T, N>(H, Di, ab, zero, [&](int j, T v) {
            mu[j] = v;
            out_tau(k, j, gd.out(v));
        });
        rnea_deriv_core<T, N>(
            mdl, cs, sn, qdv, av, true, true,
            [&](int c, const T (&col)[N]) {
                T s = lq[c];
#pragma unroll
                for (int i = 0; i < N; ++i) s = fmadd(-col[i], mu[i], s);
                lq[c] = s;
            },
            [&](int c, const T (&col)[N]) {
                T s = vb[c];
#pragma unroll
                for (int i = 0; i < N; ++i) s = fmadd(-col[i], mu[i], s);
                lv[c] = s;
            });
        extra(qv, qdv, cs, sn, mu, lq, lv);
    }
#pragma unroll
    for (int j = 0; j < N; ++j) out_state(j, gd.out(lq[j]), gd.out(lv[j]));
}

// The contact-free rollout: load_tau(k, tv) step k's torques.
template <typename T, int N, bool FAST, typename LoadTau, typename LoadG, typename WorkSt, typename WorkLd,
          typename OutTau, typename OutState>
RB_HD void rollout_vjp_eval(const T *mdl, T (&qv)[N], T (&qdv)[N], T dt, int K, LoadTau &&load_tau, LoadG &&load_g,
                            WorkSt &&work_st, WorkLd &&work_ld, OutTau &&out_tau, OutState &&out_state) {
    rollout_adjoint_eval<T, N>(
        mdl, qv, qdv, dt, K,
        [&](int k, const T (&q_)[N], const T (&v_)[N], T (&cs)[N], T (&sn)[N], T (&H)[N][N], T (&Di)[N], T (&av)[N],
            InputGuard<T> &gd) {
            vjp_step_fd<T, N, FAST>(mdl, q_, v_, [&](T (&tv)[N]) { load_tau(k, tv); }, cs, sn, H, Di, av, gd);
        },
        [](const T (&)[N], const T (&)[N], const T (&)[N], const T (&)[N], const T (&)[N], T (&)[N], T (&)[N]) {},
        static_cast<LoadG &&>(load_g), static_cast<WorkSt &&>(work_st), static_cast<WorkLd &&>(work_ld),
        static_cast<OutTau &&>(out_tau), static_cast<OutState &&>(out_state));
}

// Lane body (model-specialised kernels only, SoA rows; b: the configuration, b * sizeof(T) < 2^32).
// q, qd, g_q0, g_qd0 [n][ld]; tau_seq, gq, gqd, g_tau [K][n][ld]; work [K][2n][ld].
// eval(qv, qdv, load_tau, load_g, work_st, work_ld, out_tau, out_state): the sweeps on these rows.
template <typename T, int N, typename Eval>
__device__ __forceinline__ void rollout_adjoint_lane(const T *__restrict__ q, const T *__restrict__ qd,
                                                     const T *__restrict__ tau_seq, const T *__restrict__ gq,
                                                     const T *__restrict__ gqd, T *__restrict__ g_q0,
                                                     T *__restrict__ g_qd0, T *__restrict__ g_tau, T *work, uint32_t b,
                                                     int64_t ld, Eval &&eval) {
    const uint32_t off = b * (uint32_t)sizeof(T);
    T qv[N], qdv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        qv[j] = ld_row(q, j * ld, off);
        qdv[j] = ld_row(qd, j * ld, off);
    }
    eval(
        qv, qdv,
        [&](int k, T (&tv)[N]) {
#pragma unroll
            for (int j = 0; j < N; ++j) tv[j] = ld_row(tau_seq, ((int64_t)k * N + j) * ld, off);
        },
        [&](int k, T (&a)[N], T (&c)[N]) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                a[j] = ld_row(gq, ((int64_t)k * N + j) * ld, off);
                c[j] = ld_row(gqd, ((int64_t)k * N + j) * ld, off);
            }
        },
        [&](int k, int r, T v) { st_row(work, ((int64_t)k * (2 * N) + r) * ld, off, v); },
        [&](int k, int r) { return ld_row<T, false>(work, ((int64_t)k * (2 * N) + r) * ld, off); },
        [&](int k, int j, T v) { st_row(g_tau, ((int64_t)k * N + j) * ld, off, v); },
        [&](int j, T a, T c) {
            st_row(g_q0, j * ld, off, a);
            st_row(g_qd0, j * ld, off, c);
        });
}

template <typename T, int N, bool FAST>
__device__ __forceinline__ void rollout_vjp_lane(const T *mdl, const T *__restrict__ q, const T *__restrict__ qd,
                                                 const T *__restrict__ tau_seq, T dt, int K,
                                                 const T *__restrict__ gq, const T *__restrict__ gqd,
                                                 T *__restrict__ g_q0, T *__restrict__ g_qd0, T *__restrict__ g_tau,
                                                 T *work, uint32_t b, int64_t ld) {
    rollout_adjoint_lane<T, N>(q, qd, tau_seq, gq, gqd, g_q0, g_qd0, g_tau, work, b, ld, [&](T (&qv)[N], T (&qdv)[N], auto &&...rows) {
        rollout_vjp_eval<T, N, FAST>(mdl, qv, qdv, dt, K, static_cast<decltype(rows) &&>(rows)...);
    });
}

}  // namespace dev
}  // namespace rbamd
