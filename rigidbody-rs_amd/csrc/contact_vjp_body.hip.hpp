// contact_vjp_body.hip.hpp -- per-lane reverse-mode gradient of the fused contact rollout of serial
// revolute chains on the mass-matrix forward dynamics (host + device).
//
// The rollout (contact_body.hip.hpp rollout_contact_steps, FDH) steps, for k = 0 .. K-1,
//     fext_k = contact(q_k, v_k)      a_k = fd_ext(q_k, v_k, tau_k, fext_k)
//     v_{k+1} = v_k + dt a_k          q_{k+1} = q_k + dt v_{k+1}
// With  T(q, v, a) = rnea(q, v, a) - W(q, v),  W = sum_j J_j(q)^T fext_j(q, v)  the generalised
// contact force, the adjoint step is rollout_vjp_body.hip.hpp's with rnea replaced by T:
//     lq += gq[k];  vb = lv + gqd[k] + dt lq;  mu = sym(H(q_k))^-1 (dt vb);  g_tau[k] = mu
//     lq  = lq - (d rnea / d q)^T mu + (d W / d q)^T mu
//     lv  = vb - (d rnea / d qd)^T mu + (d W / d qd)^T mu
// The rnea terms are rollout_adjoint_eval's column sweeps, unchanged.  The contact terms are taken in
// reverse mode (contact_pullback): mu^T W = sum_p u_p . F_p(x_p, xd_p) with u_p = J_p(q) mu the
// velocity point p would have under the joint rates mu -- the cotangent of fext is link_vel(q, mu).
// In the base frame, with z_c, o_c the axis and origin of joint c, (w_c, vo_c) / (wm_c, vom_c) the
// angular velocity of link c and the velocity of o_c under the rates v / mu, and for the points on
// links >= c the sums
//     xb = (dF/dx)^T u    xdb = (dF/dxd)^T u           (contact_law_vjp, per point)
//     A1 = sum xdb   M1 = sum x x xdb   A2 = sum F   M2 = sum x x F
//     XB = sum xb    MY = sum x x xb + xd x xdb + u x F
// the derivatives are
//     d(mu^T W)/d qd_c = z_c . (M1 - o_c x A1)
//     d(mu^T W)/d q_c  = z_c . [ MY - o_c x XB - vo_c x A1 - w_c x (M1 - o_c x A1)
//                                               - vom_c x A2 - wm_c x (M2 - o_c x A2) ]
// (a point's position turns about joint c's axis, d x_p / d q_c = z_c x (x_p - o_c), and so do the
// axes and lever arms of the joints after c).  One root-to-leaf sweep -- contact_eval's own, with the
// second velocity -- evaluates the points and keeps z_c, o_c and one set of sums per link that carries
// points; one leaf-to-root loop accumulates the sums and steps the four velocities back.  Work is
// O(n + P) per step beside the column sweeps' O(n^2); nothing of size n^2 is live.
//
// The law's two max(., 0) take the derivative of the branch contact_law's own comparisons select
// (gap > 0, hc > 0): a point with f_n = 0 contributes exactly zero.  The positions and velocities
// the law sees here are contact_eval's expressions on the same (cos, sin).
//
// Forward pass: contact_fd<FDH = true>'s stages (contact_eval, rnea_ext_sweeps, the factorisation,
// the solve) and rollout_contact_steps' fmadd order, on one running InputGuard that sees q_k, v_k,
// tau_k and the wrench of every step before the backward pass stores anything; the wrench reaches
// the guard through ct_settle.  Workspace, cotangent convention and outputs: rollout_vjp_body's.
#pragma once

#include "rollout_vjp_body.hip.hpp"
#include "contact_body.hip.hpp"

namespace rbamd {
namespace dev {

template <typename T>
RB_HD T dot3(const V3<T> &a, const V3<T> &b) { return fmadd(a.x, b.x, fmadd(a.y, b.y, a.z * b.z)); }

// contact_law with its pull-back: F as there, and for a cotangent u of F
// xb = (dF/dx)^T u, xdb = (dF/dxd)^T u on the active branch (both exactly zero when f_n = 0).
template <typename T, typename Con>
RB_HD void contact_law_vjp(const Con &con, const V3<T> &x, const V3<T> &xd, const V3<T> &u, V3<T> &F, V3<T> &xb,
                           V3<T> &xdb) {
    const V3<T> nh = v3(con.normal(0), con.normal(1), con.normal(2));
    const T fn = contact_law(con, x, xd, F);
    const bool active = fn > T(0);  // hc > 0, which implies gap > 0
    const T gap = con.offset() - fmadd(nh.x, x.x, fmadd(nh.y, x.y, nh.z * x.z));
    const T phid = -fmadd(nh.x, xd.x, fmadd(nh.y, xd.y, nh.z * xd.z));
    T fnb = dot3(nh, u);  // F = f_n (nhat - mu v_t / den)
    V3<T> vtb = v3(T(0), T(0), T(0));
    if (con.friction() != T(0)) {
        const V3<T> vt = v3(fmadd(phid, nh.x, xd.x), fmadd(phid, nh.y, xd.y), fmadd(phid, nh.z, xd.z));
        const T vs = con.slip_velocity();
        const T den2 = fmadd(vt.x, vt.x, fmadd(vt.y, vt.y, fmadd(vt.z, vt.z, vs * vs)));
        const T den = ct_sqrt(den2);
        const T s = active ? con.friction() * fn / den : T(0);
        const T vu = dot3(vt, u);
        fnb = fmadd(-con.friction() / den, vu, fnb);
        const T g = vu / den2;  // d(v_t / den)/d v_t = 1 / den - v_t v_t^T / den^3
        vtb = v3(s * fmadd(g, vt.x, -u.x), s * fmadd(g, vt.y, -u.y), s * fmadd(g, vt.z, -u.z));
    }
    const T hcb = active ? fnb : T(0);  // hc = k phi (1 + c phid), phi = gap
    const T phib = hcb * con.stiffness() * fmadd(con.damping(), phid, T(1));
    const T phidb = fmadd(hcb * con.stiffness() * gap, con.damping(), dot3(vtb, nh));  // v_t = xd + phid nhat
    xdb = v3(fmadd(-phidb, nh.x, vtb.x), fmadd(-phidb, nh.y, vtb.y), fmadd(-phidb, nh.z, vtb.z));  // phid = -nhat . xd
    xb = v3(-phib * nh.x, -phib * nh.y, -phib * nh.z);                                            // gap = d - nhat . x
}

// The sums of the file comment over the points of one link, base frame.
template <typename T>
struct CvSums {
    V3<T> A1, M1, A2, M2, XB, MY;
};

template <typename T>
RB_HD void cv_add(CvSums<T> &a, const CvSums<T> &b) {
    a.A1 = add3(a.A1, b.A1); a.M1 = add3(a.M1, b.M1); a.A2 = add3(a.A2, b.A2);
    a.M2 = add3(a.M2, b.M2); a.XB = add3(a.XB, b.XB); a.MY = add3(a.MY, b.MY);
}

// acc_q(c, d(mu^T W)/d q_c), acc_v(c, d(mu^T W)/d qd_c) at the state whose joint (cos, sin) are cs / sn.
template <typename T, int N, typename Con, typename AccQ, typename AccV>
RB_HD void contact_pullback(const T *mdl, const T *ra, const Con &con, const T (&cs)[N], const T (&sn)[N],
                            const T (&qdv)[N], const T (&mu)[N], AccQ &&acc_q, AccV &&acc_v) {
    constexpr int kU = N <= kDerivUnroll ? N : 1;
    const V3<T> zero = v3(T(0), T(0), T(0));
    CvSums<T> sums[Con::kSlots];
    V3<T> zw[N], ow[N];  // joint axes and origins, base frame
    LkPose<T> X;
    LkVel<T> U, Um;  // link velocity under the rates qd / mu, link coordinates
#pragma unroll kU
    for (int j = 0; j < N; ++j) {
        const Link<T> L = load_link(mdl, j);
        const M3<T> E = joint_rotation(L.Rp, cs[j], sn[j]);
        const V3<T> r = L.p;
        if (j == 0) {  // the root link: its frame in the base, the base at rest
            X.R = E;
            X.p = r;
            U.w = U.v = Um.w = Um.v = zero;
        } else {
            const LkPose<T> P = X;
            X.p = mul_add(P.p, P.R, r);
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    X.R.m[3 * a + b] = fmadd(P.R.m[3 * a + 0], E.m[b],
                                             fmadd(P.R.m[3 * a + 1], E.m[3 + b], P.R.m[3 * a + 2] * E.m[6 + b]));
            const LkVel<T> Q = U, Qm = Um;
            U.w = mul_t(E, Q.w);
            U.v = mul_t(E, cross_sub(Q.v, r, Q.w));
            Um.w = mul_t(E, Qm.w);
            Um.v = mul_t(E, cross_sub(Qm.v, r, Qm.w));
        }
        U.w.z += qdv[j];
        Um.w.z += mu[j];
        zw[j] = v3(X.R.m[2], X.R.m[5], X.R.m[8]);
        ow[j] = X.p;
        const int slot = con.slot_of(j);
        if (slot >= 0) {
            const T *A = ra + 9 * j;
            const M3<T> Ra{{A[0], A[1], A[2], A[3], A[4], A[5], A[6], A[7], A[8]}};
            const bool turn = !lk_identity(A);
            CvSums<T> s{zero, zero, zero, zero, zero, zero};
            RB_CT_UNROLL
            for (int k = 0; k < con.points(); ++k) {
                if (con.link(k) != j) continue;
                V3<T> ck = v3(con.point(k, 0), con.point(k, 1), con.point(k, 2));
                if (turn) ck = mul_t(Ra, ck);  // x_kernel = R_a^T x_urdf
                const V3<T> x = mul_add(X.p, X.R, ck);
                const V3<T> xd = mul(X.R, cross_add(U.v, U.w, ck));
                const V3<T> u = mul(X.R, cross_add(Um.v, Um.w, ck));
                V3<T> F, xb, xdb;
                contact_law_vjp(con, x, xd, u, F, xb, xdb);
                s.A1 = add3(s.A1, xdb);
                s.M1 = cross_add(s.M1, x, xdb);
                s.A2 = add3(s.A2, F);
                s.M2 = cross_add(s.M2, x, F);
                s.XB = add3(s.XB, xb);
                s.MY = cross_add(cross_add(cross_add(s.MY, x, xb), xd, xdb), u, F);
            }
            sums[slot] = s;
        }
    }
    // the leaf's velocities in the base frame; each step back takes off one joint's share
    V3<T> w = mul(X.R, U.w), vo = mul(X.R, U.v), wm = mul(X.R, Um.w), vom = mul(X.R, Um.v);
    CvSums<T> run{zero, zero, zero, zero, zero, zero};
#pragma unroll kU
    for (int c = N - 1; c >= 0; --c) {
        const int slot = con.slot_of(c);
        if (slot >= 0) cv_add(run, sums[slot]);
        const V3<T> z = zw[c], o = ow[c];
        const V3<T> m1 = cross_sub(run.M1, o, run.A1), m2 = cross_sub(run.M2, o, run.A2);
        acc_v(c, dot3(z, m1));
        V3<T> t = cross_sub(run.MY, o, run.XB);
        t = cross_sub(cross_sub(t, vo, run.A1), w, m1);
        t = cross_sub(cross_sub(t, vom, run.A2), wm, m2);
        acc_q(c, dot3(z, t));
        if (c > 0) {
            w = v3(fmadd(-qdv[c], z.x, w.x), fmadd(-qdv[c], z.y, w.y), fmadd(-qdv[c], z.z, w.z));
            wm = v3(fmadd(-mu[c], z.x, wm.x), fmadd(-mu[c], z.y, wm.y), fmadd(-mu[c], z.z, wm.z));
            const V3<T> d = v3(o.x - ow[c - 1].x, o.y - ow[c - 1].y, o.z - ow[c - 1].z);
            vo = cross_sub(vo, w, d);  // vo_c = vo_{c-1} + w_{c-1} x (o_c - o_{c-1})
            vom = cross_sub(vom, wm, d);
        }
    }
}

// The wrench, the bias under it, H = L D L^T and a = fd_ext(q, v, tau, fext) of one step: contact_fd's
// stages (FDH) on the running check, (cos, sin) and the factors left for the backward pass.
template <typename T, int N, bool FAST, typename Topo, typename Con, typename Tau>
RB_HD void cvjp_step_fd(const T *mdl, const T *ra, const Con &con, const T (&qv)[N], const T (&qdv)[N], Tau &&load_tau,
                        T (&cs)[N], T (&sn)[N], T (&H)[N][N], T (&Di)[N], T (&av)[N], InputGuard<T> &gd) {
    T fw[Con::kSlots][6];
    contact_eval<T, N, FAST, Topo>(mdl, ra, con, qv, qdv, fw, [](int, T) {});
    auto fx = [&](int r) {
        const int slot = con.slot_of(r / 6);
        return slot >= 0 ? ct_settle(fw[slot][r % 6]) : T(0);
    };
    T C[N], tv[N];
    rnea_ext_sweeps<T, N, FAST, Topo, false>(mdl, ra, qv, qdv, qdv /* unread */, fx, cs, sn, gd,
                                             [&](int j, T v) { C[j] = v; });
    load_tau(tv);
    fdh_factor<T, N>(mdl, cs, sn, H, Di);
    gd.vals(tv);
    fdh_solve<T, N>(H, Di, tv, C, [&](int j, T v) { av[j] = v; });
}

// rollout_vjp_eval's arguments, with the contact set and the links' axis frames.
template <typename T, int N, bool FAST, typename Topo, typename Con, typename LoadTau, typename LoadG, typename WorkSt,
          typename WorkLd, typename OutTau, typename OutState>
RB_HD void rollout_contact_vjp_eval(const T *mdl, const T *ra, const Con &con, T (&qv)[N], T (&qdv)[N], T dt, int K,
                                    LoadTau &&load_tau, LoadG &&load_g, WorkSt &&work_st, WorkLd &&work_ld,
                                    OutTau &&out_tau, OutState &&out_state) {
    rollout_adjoint_eval<T, N>(
        mdl, qv, qdv, dt, K,
        [&](int k, const T (&q_)[N], const T (&v_)[N], T (&cs)[N], T (&sn)[N], T (&H)[N][N], T (&Di)[N], T (&av)[N],
            InputGuard<T> &gd) {
            cvjp_step_fd<T, N, FAST, Topo>(mdl, ra, con, q_, v_, [&](T (&tv)[N]) { load_tau(k, tv); }, cs, sn, H, Di, av,
                                           gd);
        },
        [&](const T (&)[N], const T (&v_)[N], const T (&cs)[N], const T (&sn)[N], const T (&mu)[N], T (&lq)[N],
            T (&lv)[N]) {
            contact_pullback<T, N>(
                mdl, ra, con, cs, sn, v_, mu, [&](int c, T g) { lq[c] += g; }, [&](int c, T g) { lv[c] += g; });
        },
        static_cast<LoadG &&>(load_g), static_cast<WorkSt &&>(work_st), static_cast<WorkLd &&>(work_ld),
        static_cast<OutTau &&>(out_tau), static_cast<OutState &&>(out_state));
}

// Lane body: rollout_vjp_lane's rows.
template <typename T, int N, bool FAST, typename Topo, typename Con>
__device__ __forceinline__ void rollout_contact_vjp_lane(const T *mdl, const T *ra, const T *__restrict__ q,
                                                         const T *__restrict__ qd, const T *__restrict__ tau_seq, T dt,
                                                         int K, const T *__restrict__ gq, const T *__restrict__ gqd,
                                                         T *__restrict__ g_q0, T *__restrict__ g_qd0,
                                                         T *__restrict__ g_tau, T *work, uint32_t b, int64_t ld) {
    rollout_adjoint_lane<T, N>(q, qd, tau_seq, gq, gqd, g_q0, g_qd0, g_tau, work, b, ld,
                               [&](T (&qv)[N], T (&qdv)[N], auto &&...rows) {
                                   rollout_contact_vjp_eval<T, N, FAST, Topo>(mdl, ra, Con{}, qv, qdv, dt, K,
                                                                              static_cast<decltype(rows) &&>(rows)...);
                               });
}

}  // namespace dev
}  // namespace rbamd
