// fd_vjp_body.hip.hpp -- reverse-mode gradient of the forward dynamics (device + host).
//
//   qdd = fd_ext(q, qd, tau, fext)       (ext_body.hip.hpp; EXT = false: no wrench rows, fext = 0 in registers)
//   L   = sum_i w_i qdd_i                (w: the cotangent of qdd)
//   mu  = sym(H(q))^-1 w
//   g_tau = mu,  (g_q, g_qd, ., g_fext) = -rnea_vjp(q, qd, qdd, fext; cotangent mu)
// because H dqdd + d rnea_ext(q, qd, qdd, fext) = dtau at fixed qdd.  So g_fext_j = +J_j(q) mu, what
// link_vel(q, mu) returns for link j.
//
// Two stages per lane over the `Topo` policy; only q, qd, qdd and mu cross from one to the other.
//
// Stage 1 is the forward dynamics in the form fd_ext takes for the model (FDH: the mass-matrix form,
// else the ABA), with a second right-hand side: the same operations in the same order give qdd, and
// the one factorisation also solves sym(H) mu = w.
//   mass-matrix form  rnea_ext_sweeps<QDD = false> (the bias C), fdh_factor (serial chains) or
//                     crba_eval_tree + fdh_ldl (trees), then fdh_solve twice: (tau, C) and (w, 0).
//   ABA               aba_ext_eval's three passes (fd2_aba below).  The second right-hand side has no
//                     velocity products, no wrench and a base at rest, so pass 2 carries a second
//                     bias-force accumulator and a second u / D per link and pass 3 a second
//                     acceleration; U / D, 1 / D and the articulated inertias are computed once.
// Stage 2 is rnea_vjp_eval (rnea_vjp_body.hip.hpp) at qddv = qdd, wv = mu, its outputs negated.
//
// The wrench rows are fetched by the link step that consumes them in each stage, so they are read
// twice and the 6 n values are never held together.  Every input (q, qd, tau, fext) has gone through
// stage 1's InputGuard when qdd and g_tau -- the first stores -- leave; stage 2 sees the guarded qdd
// and checks q, qd and the wrench rows again, so an out-of-domain configuration gets NaN everywhere.
// The cotangent w is not checked.
#pragma once

#include "rnea_vjp_body.hip.hpp"

namespace rbamd {
namespace dev {

// aba_ext_eval (ext_body.hip.hpp) with the second right-hand side (wv, no bias, base at rest):
// qddv = the ABA's accelerations, operation for operation; muv = H^-1 wv.  Raw values: the caller
// applies gd.
template <typename T, int N, bool FAST, typename Topo, typename Fx>
RB_HD void fd2_aba(const T *mdl, const T *ra, const T (&qv)[N], const T (&qdv)[N], const T (&tv)[N], const T (&wv)[N],
                   Fx &&fx, InputGuard<T> &gd, T (&qddv)[N], T (&muv)[N]) {
    gd.vals(tv);
    T cs[N], sn[N];
    V3<T> W[N], V[N];                  // pass-1 velocities (read by children)
    T cw0[N], cw1[N], cv0[N], cv1[N];  // c_i = v_i x (S qd_i), nonzero entries
    V3<T> pn[N], pf[N];                // bias forces p_i = v_i x* (I_i v_i) - fext_i
    cfor<0, N>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr int p = Topo::parent(j);
        constexpr bool pri = Topo::prismatic(j);
        const Link<T> L = load_link(mdl, j);
        const T qdj = qdv[j];
        if constexpr (pri) gd.val(qv[j]); else gd.angle(qv[j]);
        gd.val(qdj);
        if constexpr (!pri) sin_cos<FAST>(qv[j], sn[j], cs[j]); else { cs[j] = T(1); sn[j] = T(0); }
        V3<T> w, v;
        if constexpr (p < 0) {
            w = v3(T(0), T(0), T(0));
            v = w;
        } else {
            M3<T> E;
            V3<T> r;
            link_frame<T, pri>(L, qv[j], cs[j], sn[j], E, r);
            w = mul_t(E, W[p]);
            v = mul_t(E, cross_sub(V[p], r, W[p]));
        }
        if constexpr (!pri) {
            w.z += qdj;
            cw0[j] = w.y * qdj; cw1[j] = -w.x * qdj;
            cv0[j] = v.y * qdj; cv1[j] = -v.x * qdj;
        } else {
            v.z += qdj;
            cw0[j] = T(0); cw1[j] = T(0);
            cv0[j] = w.y * qdj; cv1[j] = -w.x * qdj;
        }
        W[j] = w;
        V[j] = v;
        V3<T> In, If, xn, xf;
        inertia_mul(L, w, v, In, If);
        ext_wrench(ra, j, fx, gd, xn, xf);
        const V3<T> f = cross(w, If);
        const V3<T> n = cross_add(cross(w, In), v, If);
        pf[j] = v3(f.x - xf.x, f.y - xf.y, f.z - xf.z);
        pn[j] = v3(n.x - xn.x, n.y - xn.y, n.z - xn.z);
    });

    reload_fence();
    ArtI<T> IAc[N];        // articulated inertia accumulators (a parent's, from its children)
    V3<T> pAn[N], pAf[N];  // bias force accumulators
    V3<T> qAn[N], qAf[N];  // ... of the second right-hand side (a link's own bias force is zero)
    V3<T> UrD[N], UlD[N];  // U / D (its S-component is exactly 1)
    T uD[N], uD2[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        qAn[j] = v3(T(0), T(0), T(0));
        qAf[j] = qAn[j];
    }
    cfor_rev<N>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr int p = Topo::parent(j);
        constexpr bool pri = Topo::prismatic(j);
        const Link<T> L = load_link(mdl, j);
        ArtI<T> IA;
        V3<T> An, Af;
        if constexpr (ext_last_child<Topo, N>(j) < 0) {  // a leaf: its own rigid inertia
            IA = rigid_inertia(L);
            An = pn[j];
            Af = pf[j];
        } else {
            IA = IAc[j];
            An = pAn[j];
            Af = pAf[j];
        }
        const V3<T> Bn = qAn[j], Bf = qAf[j];
        V3<T> ur, ul;
        T D, u, u2;
        if constexpr (!pri) {
            ur = v3(IA.A.xz, IA.A.yz, IA.A.zz);
            ul = v3(IA.B.m[6], IA.B.m[7], IA.B.m[8]);
            D = IA.A.zz;
            u = tv[j] - An.z;
            u2 = wv[j] - Bn.z;
        } else {
            ur = v3(IA.B.m[2], IA.B.m[5], IA.B.m[8]);
            ul = v3(IA.M.xz, IA.M.yz, IA.M.zz);
            D = IA.M.zz;
            u = tv[j] - Af.z;
            u2 = wv[j] - Bf.z;
        }
        const T Dinv = recip(D);
        V3<T> dr = v3(ur.x * Dinv, ur.y * Dinv, ur.z * Dinv);
        V3<T> dl = v3(ul.x * Dinv, ul.y * Dinv, ul.z * Dinv);
        if constexpr (!pri) dr.z = T(1); else dl.z = T(1);
        UrD[j] = dr;
        UlD[j] = dl;
        uD[j] = u * Dinv;
        uD2[j] = u2 * Dinv;
        if constexpr (p >= 0) {
            ArtI<T> Ia;
            Ia.A = S3<T>{fmadd(-ur.x, dr.x, IA.A.xx), fmadd(-ur.x, dr.y, IA.A.xy), fmadd(-ur.x, dr.z, IA.A.xz),
                         fmadd(-ur.y, dr.y, IA.A.yy), fmadd(-ur.y, dr.z, IA.A.yz), fmadd(-ur.z, dr.z, IA.A.zz)};
#pragma unroll
            for (int rr = 0; rr < 3; ++rr) {
                const T urr = rr == 0 ? ur.x : (rr == 1 ? ur.y : ur.z);
                Ia.B.m[3 * rr + 0] = fmadd(-urr, dl.x, IA.B.m[3 * rr + 0]);
                Ia.B.m[3 * rr + 1] = fmadd(-urr, dl.y, IA.B.m[3 * rr + 1]);
                Ia.B.m[3 * rr + 2] = fmadd(-urr, dl.z, IA.B.m[3 * rr + 2]);
            }
            Ia.M = S3<T>{fmadd(-ul.x, dl.x, IA.M.xx), fmadd(-ul.x, dl.y, IA.M.xy), fmadd(-ul.x, dl.z, IA.M.xz),
                         fmadd(-ul.y, dl.y, IA.M.yy), fmadd(-ul.y, dl.z, IA.M.yz), fmadd(-ul.z, dl.z, IA.M.zz)};
            if constexpr (!pri) {  // Ia (e_z; 0) = 0: A's z row/column, B's z row
                Ia.A.xz = T(0); Ia.A.yz = T(0); Ia.A.zz = T(0);
                Ia.B.m[6] = T(0); Ia.B.m[7] = T(0); Ia.B.m[8] = T(0);
            } else {  // Ia (0; e_z) = 0: B's z column, M's z row/column
                Ia.B.m[2] = T(0); Ia.B.m[5] = T(0); Ia.B.m[8] = T(0);
                Ia.M.xz = T(0); Ia.M.yz = T(0); Ia.M.zz = T(0);
            }
            // pa = pA + Ia c + U u / D, c = (cw0, cw1, 0; cv0, cv1, 0)
            const V3<T> cr = v3(cw0[j], cw1[j], T(0)), cl = v3(cv0[j], cv1[j], T(0));
            const V3<T> uu = v3(ur.x * uD[j], ur.y * uD[j], ur.z * uD[j]);
            const V3<T> lu = v3(ul.x * uD[j], ul.y * uD[j], ul.z * uD[j]);
            V3<T> pa_n = add3(mul_add(mul_add(An, Ia.A, cr), Ia.B, cl), uu);
            V3<T> pa_f = add3(add3(mul_add(Af, Ia.M, cl), mul_t(Ia.B, cr)), lu);
            // the second right-hand side: c = 0, so pa = pA + U u2 / D
            V3<T> qa_n = v3(fmadd(ur.x, uD2[j], Bn.x), fmadd(ur.y, uD2[j], Bn.y), fmadd(ur.z, uD2[j], Bn.z));
            V3<T> qa_f = v3(fmadd(ul.x, uD2[j], Bf.x), fmadd(ul.y, uD2[j], Bf.y), fmadd(ul.z, uD2[j], Bf.z));
            M3<T> E;
            V3<T> r;
            link_frame<T, pri>(L, qv[j], cs[j], sn[j], E, r);
            force_to_parent(E, r, pa_n, pa_f);
            force_to_parent(E, r, qa_n, qa_f);
            const ArtI<T> moved = to_parent(E, r, Ia);
            if constexpr (ext_last_child<Topo, N>(p) == j) {  // first contribution (highest child)
                IAc[p] = moved;
                add_rigid(IAc[p], load_link(mdl, p));
                pAn[p] = add3(pn[p], pa_n);
                pAf[p] = add3(pf[p], pa_f);
            } else {
                add_art(IAc[p], moved);
                pAn[p] = add3(pAn[p], pa_n);
                pAf[p] = add3(pAf[p], pa_f);
            }
            qAn[p] = add3(qAn[p], qa_n);
            qAf[p] = add3(qAf[p], qa_f);
        }
    });

    reload_fence();
    V3<T> AW[N], AV[N];  // link accelerations
    V3<T> BW[N], BV[N];  // ... of the second right-hand side
    cfor<0, N>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr int p = Topo::parent(j);
        constexpr bool pri = Topo::prismatic(j);
        const Link<T> L = load_link(mdl, j);
        M3<T> E;
        V3<T> r;
        link_frame<T, pri>(L, qv[j], cs[j], sn[j], E, r);
        V3<T> aw, av, bw, bv;
        if constexpr (p < 0) {
            const T g = T(kGravity);
            aw = v3(T(0), T(0), T(0));
            av = v3(g * E.m[6], g * E.m[7], g * E.m[8]);
            bw = aw;
            bv = aw;
        } else {
            aw = mul_t(E, AW[p]);
            av = mul_t(E, cross_sub(AV[p], r, AW[p]));
            bw = mul_t(E, BW[p]);
            bv = mul_t(E, cross_sub(BV[p], r, BW[p]));
        }
        aw.x += cw0[j]; aw.y += cw1[j];
        av.x += cv0[j]; av.y += cv1[j];
        const V3<T> dr = UrD[j], dl = UlD[j];
        const T a = uD[j] - fmadd(dr.x, aw.x, fmadd(dr.y, aw.y, fmadd(dr.z, aw.z,
                                  fmadd(dl.x, av.x, fmadd(dl.y, av.y, dl.z * av.z)))));
        const T a2 = uD2[j] - fmadd(dr.x, bw.x, fmadd(dr.y, bw.y, fmadd(dr.z, bw.z,
                                    fmadd(dl.x, bv.x, fmadd(dl.y, bv.y, dl.z * bv.z)))));
        if constexpr (!pri) { aw.z += a; bw.z += a2; } else { av.z += a; bv.z += a2; }
        AW[j] = aw;
        AV[j] = av;
        BW[j] = bw;
        BV[j] = bv;
        qddv[j] = a;
        muv[j] = a2;
    });
}

// fdh_ext_eval (ext_body.hip.hpp) with the second right-hand side solved on the same factorisation.
// load_tw(tv, wv) fetches tau and w after the bias sweep, as fdh_ext_eval fetches tau.
template <typename T, int N, bool FAST, typename Topo, typename Fx, typename LoadTW>
RB_HD void fd2_fdh(const T *mdl, const T *ra, const T (&qv)[N], const T (&qdv)[N], Fx &&fx, LoadTW &&load_tw,
                   InputGuard<T> &gd, T (&qddv)[N], T (&muv)[N]) {
    T cs[N], sn[N], C[N], tv[N], wv[N], zero[N], H[N][N], Di[N];
    rnea_ext_sweeps<T, N, FAST, Topo, false>(mdl, ra, qv, qdv, qdv /* unread */, fx, cs, sn, gd,
                                             [&](int j, T v) { C[j] = v; });
    load_tw(tv, wv);
    if constexpr (Topo::kSerial) {
        fdh_factor<T, N>(mdl, cs, sn, H, Di);
    } else {
        reload_fence();
        crba_eval_tree<T, N, FAST, Topo>(mdl, qv, [&](int e, T v) {
            const int j = e % N, i = e / N;
            if (j <= i) H[j][i] = v;
        });
        fdh_ldl<T, N>(H, Di);
    }
    gd.vals(tv);
#pragma unroll
    for (int j = 0; j < N; ++j) zero[j] = T(0);
    fdh_solve<T, N>(H, Di, tv, C, [&](int j, T v) { qddv[j] = v; });
    fdh_solve<T, N>(H, Di, wv, zero, [&](int j, T v) { muv[j] = v; });
}

// fx(row): wrench row of this configuration (EXT only; called once per row in each stage).
// load_tw(tv, wv): fetches tau and w (the ABA form calls it first, the mass-matrix form after its
// bias sweep).  want_f: g_fext is asked for.  out_qdd / out_tau / out_q / out_qd (j, value) over N
// rows, out_f(row, value) over 6 N rows; qdd and g_tau leave root first, the others leaf first.
template <typename T, int N, bool FAST, typename Topo, bool EXT, bool FDH, typename Fx, typename LoadTW, typename OQdd,
          typename OQ, typename OQd, typename OTau, typename OF>
RB_HD void fd_vjp_eval(const T *mdl, const T *ra, const T (&qv)[N], const T (&qdv)[N], Fx &&fx, LoadTW &&load_tw,
                       bool want_f, OQdd &&out_qdd, OQ &&out_q, OQd &&out_qd, OTau &&out_tau, OF &&out_f) {
    // EXT = false runs the wrench form's own arithmetic on a zero the compiler cannot see through: were the
    // zero folded away, the link forces' last multiplies would fuse with other additions than they do next
    // to a wrench, and the results would differ from the wrench family's at fext = 0 in the last bit.
    T zero = T(0);
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC_RTC__)
    asm("" : "+v"(zero));
#endif
    auto row = [&](int r) {
        if constexpr (EXT)
            return fx(r);
        else
            return zero;
    };
    T qddv[N], muv[N];
    {
        InputGuard<T> gd;
        if constexpr (FDH) {
            fd2_fdh<T, N, FAST, Topo>(mdl, ra, qv, qdv, row, load_tw, gd, qddv, muv);
        } else {
            T tv[N], wv[N];
            load_tw(tv, wv);
            fd2_aba<T, N, FAST, Topo>(mdl, ra, qv, qdv, tv, wv, row, gd, qddv, muv);
        }
#pragma unroll
        for (int j = 0; j < N; ++j) {
            qddv[j] = gd.out(qddv[j]);
            muv[j] = gd.out(muv[j]);
            out_qdd(j, qddv[j]);
            out_tau(j, muv[j]);
        }
    }
    reload_fence();
    rnea_vjp_eval<T, N, FAST, Topo, true>(
        mdl, ra, qv, qdv, qddv, muv, row, EXT && want_f, [&](int j, T v) { out_q(j, -v); },
        [&](int j, T v) { out_qd(j, -v); }, [](int, T) {}, [&](int r, T v) { out_f(r, -v); });
}

// ---------------------------------------------------------------------- lane body
// One configuration per lane on SoA rows.  q and qd are loaded up front and tau, w where fd_ext_lane
// loads tau; the wrench rows by the link step that consumes them in each stage (EXT only), under the
// same RB_NT policy as fd_ext_lane.  EXT = false never touches fext / g_fext.
template <typename T, int N, bool FAST, typename Topo, bool EXT, bool FDH>
__device__ __forceinline__ void fd_vjp_lane(const T *mdl, const T *ra, const T *__restrict__ q,
                                            const T *__restrict__ qd, const T *__restrict__ tau,
                                            const T *__restrict__ fext, const T *__restrict__ w,
                                            T *__restrict__ qdd, T *__restrict__ g_q, T *__restrict__ g_qd,
                                            T *__restrict__ g_tau, T *__restrict__ g_fext, uint32_t b, int64_t ld) {
    const uint32_t off = b * (uint32_t)sizeof(T);
    T qv[N], qdv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        qv[j] = ld_row(q, j * ld, off);
        __builtin_amdgcn_sched_barrier(0);
        qdv[j] = ld_row(qd, j * ld, off);
        __builtin_amdgcn_sched_barrier(0);
    }
    // each wrench row is read once per stage: a temporal load whatever RB_NT says, so that the second read
    // can be served from cache (not measured against the non-temporal form)
    auto fx = [&](int r) { return ld_row<T, false>(fext, r * ld, off); };
    auto load_tw = [&](T (&tv)[N], T (&wv)[N]) {
        if constexpr (FDH) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                tv[j] = ld_row(tau, j * ld, off);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int j = N - 1; j >= 0; --j) {
                tv[j] = ld_row(tau, j * ld, off);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int j = 0; j < N; ++j) wv[j] = ld_row(w, j * ld, off);
    };
    fd_vjp_eval<T, N, FAST, Topo, EXT, FDH>(
        mdl, ra, qv, qdv, fx, load_tw, EXT, [&](int j, T v) { st_row(qdd, j * ld, off, v); },
        [&](int j, T v) { st_row(g_q, j * ld, off, v); }, [&](int j, T v) { st_row(g_qd, j * ld, off, v); },
        [&](int j, T v) { st_row(g_tau, j * ld, off, v); }, [&](int r, T v) { st_row(g_fext, r * ld, off, v); });
}

}  // namespace dev
}  // namespace rbamd
