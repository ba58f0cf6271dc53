// rnea_deriv_body.hip.hpp -- per-lane analytical derivatives of the inverse and forward
// dynamics of serial revolute chains (host + device).
//
//   dtau_dq [i, k] = d rnea(q, qd, qdd)_i / d q_k      dtau_dqd[i, k] = d rnea_i / d qd_k
//   dqdd_dq = -sym(H)^-1 dtau_dq(q, qd, qdd),  dqdd_dqd = -sym(H)^-1 dtau_dqd(q, qd, qdd),
//   dqdd_dtau = sym(H)^-1                      with qdd = fd(q, qd, tau) (fdh_body.hip.hpp)
//
// One configuration per lane, forward-mode (tangent) sweeps of the RNEA recursion
// (multibody.rs:111-153), one differentiated joint k at a time:
//   * q_k enters only through E_k = R_p,k Rz(q_k).  Forward step: d(E^T x)/dq = -z x (E^T x), and the
//     joint's own z qd, z qdd terms are invariant under it, so at link k every kinematic vector
//     x in (w, v, aw, av) has the tangent -z x x = (x.y, -x.x, 0); links j < k have none.
//     Backward step: d(E F)/dq = E (z x F) with F the wrench link k transmits.
//   * qd_k enters at link k as dw = z, daw = w x z, dav = v x z (v_k does not depend on qd_k).
//   * links j > k propagate either tangent by the primal step without its joint terms; every
//     link's wrench tangent is the differential of link_force; the backward sweep runs over all
//     links (ancestors' torques depend on q_k through the transmitted wrench).
// Column k (n values per output) leaves as soon as it is complete: no n^2 accumulator is live.
//
// Primal state.  The link kinematics K_j (12 values per link) are evaluated once and kept across
// the column sweeps; the columns run leaf first so that the primal transmitted wrench F_k -- needed
// by column k alone -- is carried in 6 values, F_k = f_k + X_{k+1} F_{k+1}, the link force f_k
// re-evaluated from K_k.  Per column the wrench tangents of links k.. are held for the backward
// sweep (6 (n - k) values).  DESIGN.md has the register counts of this form and of the two
// alternatives (recomputing K_j alongside each tangent, parking it in LDS).
#pragma once

#include "spatial.hip.hpp"

#if !defined(__HIPCC_RTC__)
namespace rbamd {
namespace dev {
// fdh_ldl's reciprocal on the host (the device forms are hardware reciprocals, spatial.hip.hpp)
__host__ inline double recip(double x) { return 1.0 / x; }
}  // namespace dev
}  // namespace rbamd
#endif

#include "fdh_body.hip.hpp"

namespace rbamd {
namespace dev {

// Column sweeps are unrolled (every per-link value a register) up to this many links; longer
// chains run them as loops over per-lane arrays (slow, but any serial chain evaluates).
constexpr int kDerivUnroll = 16;

// -z x x: the tangent of a link-frame vector under the joint's own rotation
template <typename T>
RB_HD V3<T> rot_z_tan(const V3<T> &x) { return v3(x.y, -x.x, T(0)); }

// One forward step of the primal kinematics on given (cos, sin) (rnea_fwd's arithmetic without the
// link force; link 0 takes the base state w = v = aw = 0, av = (0, 0, g)).
template <typename T>
RB_HD void deriv_fwd(const T *mdl, int j, T cj, T sj, T qdj, T qddj, const RneaState<T> &p, RneaState<T> &s) {
    const Link<T> L = load_link(mdl, j);
    const M3<T> E = joint_rotation(L.Rp, cj, sj);
    const V3<T> u = cross_sub(p.v, L.p, p.w);
    const V3<T> ua = cross_sub(p.av, L.p, p.aw);
    V3<T> wn = mul_t(E, p.w), vn = mul_t(E, u);
    V3<T> awn = mul_t(E, p.aw), avn = mul_t(E, ua);
    wn.z += qdj;
    awn.z += qddj;
    avn.x = fmadd(vn.y, qdj, avn.x);
    avn.y = fmadd(-vn.x, qdj, avn.y);
    awn.x = fmadd(wn.y, qdj, awn.x);
    awn.y = fmadd(-wn.x, qdj, awn.y);
    s.w = wn; s.v = vn; s.aw = awn; s.av = avn;
}

// The same step on a tangent: linear in the parent's tangent, no joint terms of its own (j > k).
template <typename T>
RB_HD void deriv_fwd_tan(const T *mdl, int j, T cj, T sj, T qdj, RneaState<T> &d) {
    const Link<T> L = load_link(mdl, j);
    const M3<T> E = joint_rotation(L.Rp, cj, sj);
    const V3<T> u = cross_sub(d.v, L.p, d.w);
    const V3<T> ua = cross_sub(d.av, L.p, d.aw);
    V3<T> wn = mul_t(E, d.w), vn = mul_t(E, u);
    V3<T> awn = mul_t(E, d.aw), avn = mul_t(E, ua);
    avn.x = fmadd(vn.y, qdj, avn.x);
    avn.y = fmadd(-vn.x, qdj, avn.y);
    awn.x = fmadd(wn.y, qdj, awn.x);
    awn.y = fmadd(-wn.x, qdj, awn.y);
    d.w = wn; d.v = vn; d.aw = awn; d.av = avn;
}

// Differential of link_force (spatial.hip.hpp) at the link state s along the tangent d.
#if RB_COM_FORM
template <typename T>
RB_HD void link_force_tan(const Link<T> &L, int j, const RneaState<T> &s, const RneaState<T> &d, V3<T> &dfn,
                          V3<T> &dff) {
    const double *k = rb_com + 9 * j;
    const V3<T> c = v3(com_k<T>(k[0]), com_k<T>(k[1]), com_k<T>(k[2]));
    const S3<T> Ic{com_k<T>(k[3]), com_k<T>(k[4]), com_k<T>(k[5]), com_k<T>(k[6]), com_k<T>(k[7]), com_k<T>(k[8])};
    const V3<T> vc = cross_add(s.v, s.w, c);
    const V3<T> dvc = cross_add(d.v, d.w, c);
    // g = av + aw x c + w x vc
    const V3<T> dg = cross_add(cross_add(cross_add(d.av, d.aw, c), d.w, vc), s.w, dvc);
    dff = v3(L.m * dg.x, L.m * dg.y, L.m * dg.z);
    // n = Ic aw + w x (Ic w) + c x f
    dfn = cross_add(cross_add(cross_add(mul(Ic, d.aw), d.w, mul(Ic, s.w)), s.w, mul(Ic, d.w)), c, dff);
}
#else
template <typename T>
RB_HD void link_force_tan(const Link<T> &L, int, const RneaState<T> &s, const RneaState<T> &d, V3<T> &dfn,
                          V3<T> &dff) {
    V3<T> In, If, dIn, dIf, An, Af;
    inertia_mul(L, s.w, s.v, In, If);
    inertia_mul(L, d.w, d.v, dIn, dIf);
    inertia_mul(L, d.aw, d.av, An, Af);
    // f = Af + w x If,  n = An + w x In + v x If
    dff = cross_add(cross_add(Af, d.w, If), s.w, dIf);
    dfn = cross_add(cross_add(cross_add(cross_add(An, d.w, In), s.w, dIn), d.v, If), s.v, dIf);
}
#endif

// One column: the tangent sweeps for joint k.  QD = false: d/dq_k, true: d/dqd_k.  K: the primal
// link kinematics; (Fn, Ff): the wrench link k transmits (d/dq_k only).  col[i] = d tau_i.
template <typename T, int N, bool QD>
RB_HD void deriv_column(const T *mdl, int k, const T (&cs)[N], const T (&sn)[N], const T (&qdv)[N],
                        const RneaState<T> (&K)[N], const V3<T> &Fn, const V3<T> &Ff, T (&col)[N]) {
    constexpr int kU = N <= kDerivUnroll ? N : 1;
    V3<T> dfn[N], dff[N];  // wrench tangents; links j < k have none of their own
    RneaState<T> d;
    if constexpr (QD) {
        d.w = v3(T(0), T(0), T(1));
        d.v = v3(T(0), T(0), T(0));
        d.aw = rot_z_tan(K[k].w);  // w x z
        d.av = rot_z_tan(K[k].v);  // v x z
    } else {
        d.w = rot_z_tan(K[k].w);
        d.v = rot_z_tan(K[k].v);
        d.aw = rot_z_tan(K[k].aw);
        d.av = rot_z_tan(K[k].av);
    }
#pragma unroll kU
    for (int j = 0; j < N; ++j) {
        if (j < k) {
            dfn[j] = v3(T(0), T(0), T(0));
            dff[j] = v3(T(0), T(0), T(0));
            continue;
        }
        if (j > k) deriv_fwd_tan(mdl, j, cs[j], sn[j], qdv[j], d);
        link_force_tan(load_link(mdl, j), j, K[j], d, dfn[j], dff[j]);
    }
    reload_fence();
#pragma unroll kU
    for (int j = N - 1; j >= 1; --j) {
        col[j] = dfn[j].z;
        V3<T> tn = dfn[j], tf = dff[j];
        if (!QD && j == k) {  // d(E F)/dq = E (z x F): the rotated primal wrench joins the tangent
            tn = v3(tn.x - Fn.y, tn.y + Fn.x, tn.z);
            tf = v3(tf.x - Ff.y, tf.y + Ff.x, tf.z);
        }
        rnea_bwd(mdl, j, cs[j], sn[j], tf, tn, dff[j - 1], dfn[j - 1]);
    }
    col[0] = dfn[0].z;
}

// Both derivative matrices of rnea(q, qd, qdd) on given joint (cos, sin).  colq(k, col) /
// colqd(k, col) receive column k (col[i] = d tau_i / d q_k, d tau_i / d qd_k), k = n-1 .. 0; a
// matrix that is not wanted is not evaluated.
template <typename T, int N, typename ColQ, typename ColQd>
RB_HD void rnea_deriv_core(const T *mdl, const T (&cs)[N], const T (&sn)[N], const T (&qdv)[N], const T (&qddv)[N],
                           bool want_q, bool want_qd, ColQ &&colq, ColQd &&colqd) {
    constexpr int kU = N <= kDerivUnroll ? N : 1;
    RneaState<T> K[N];
    {
        RneaState<T> base;
        base.w = v3(T(0), T(0), T(0));
        base.v = v3(T(0), T(0), T(0));
        base.aw = v3(T(0), T(0), T(0));
        base.av = v3(T(0), T(0), T(kGravity));
        deriv_fwd(mdl, 0, cs[0], sn[0], qdv[0], qddv[0], base, K[0]);
    }
#pragma unroll kU
    for (int j = 1; j < N; ++j) deriv_fwd(mdl, j, cs[j], sn[j], qdv[j], qddv[j], K[j - 1], K[j]);
    V3<T> Fn = v3(T(0), T(0), T(0)), Ff = Fn;  // the wrench link k transmits, in link k's frame
#pragma unroll kU
    for (int k = N - 1; k >= 0; --k) {
        reload_fence();
        if (want_q) {
            V3<T> fn, ff;
            link_force(load_link(mdl, k), k, K[k].w, K[k].v, K[k].aw, K[k].av, fn, ff);
            if (k < N - 1) rnea_bwd(mdl, k + 1, cs[k + 1], sn[k + 1], Ff, Fn, ff, fn);
            Fn = fn;
            Ff = ff;
            T col[N];
            deriv_column<T, N, false>(mdl, k, cs, sn, qdv, K, Fn, Ff, col);
            colq(k, col);
        }
        if (want_qd) {
            T col[N];
            deriv_column<T, N, true>(mdl, k, cs, sn, qdv, K, Fn, Ff, col);
            colqd(k, col);
        }
    }
}

// rnea derivatives of one configuration: input checks (InputGuard: an out-of-domain input makes
// every output element NaN), the joint sincos, then the column sweeps.  outq(e, v) / outqd(e, v):
// element e = i + n k of the column-major matrices.
template <typename T, int N, bool FAST, typename OutQ, typename OutQd>
RB_HD void rnea_deriv_eval(const T *mdl, const T (&qv)[N], const T (&qdv)[N], const T (&qddv)[N], bool want_q,
                           bool want_qd, OutQ &&outq, OutQd &&outqd) {
    InputGuard<T> gd;
    T cs[N], sn[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        gd.angle(qv[j]);
        gd.val(qdv[j]);
        gd.val(qddv[j]);
        sin_cos<FAST>(qv[j], sn[j], cs[j]);
    }
    rnea_deriv_core<T, N>(
        mdl, cs, sn, qdv, qddv, want_q, want_qd,
        [&](int k, const T (&col)[N]) {
#pragma unroll
            for (int i = 0; i < N; ++i) outq(i + N * k, gd.out(col[i]));
        },
        [&](int k, const T (&col)[N]) {
#pragma unroll
            for (int i = 0; i < N; ++i) outqd(i + N * k, gd.out(col[i]));
        });
}

// Forward dynamics and its derivatives of one configuration (mass-matrix form): the bias, H and
// L D L^T once, qdd by fdh_eval's own steps (bit-identical to the forward-dynamics kernel), then
// every tangent column of rnea at (q, qd, qdd) and every unit vector back-substituted through the
// kept factors.  out_qdd(j, v); out_dq / out_dqd / out_dtau(e, v), e = i + n k.
template <typename T, int N, bool FAST, typename Tau, typename OutA, typename OutQ, typename OutQd, typename OutTau>
RB_HD void fd_deriv_eval(const T *mdl, const T (&qv)[N], const T (&qdv)[N], Tau &&load_tau, bool want_q, bool want_qd,
                         bool want_tau, OutA &&out_qdd, OutQ &&out_dq, OutQd &&out_dqd, OutTau &&out_dtau) {
    constexpr int kU = N <= kDerivUnroll ? N : 1;
    T cs[N], sn[N], C[N], tv[N], av[N], H[N][N], Di[N];
    InputGuard<T> gd;
    fdh_bias<T, N, FAST>(mdl, qv, qdv, cs, sn, C, gd);
    load_tau(tv);
    fdh_factor<T, N>(mdl, cs, sn, H, Di);
    gd.vals(tv);
    fdh_solve<T, N>(H, Di, tv, C, [&](int j, T v) {
        av[j] = v;
        out_qdd(j, gd.out(v));
    });
    T zero[N];
#pragma unroll
    for (int j = 0; j < N; ++j) zero[j] = T(0);
    if (want_q || want_qd) {
        rnea_deriv_core<T, N>(
            mdl, cs, sn, qdv, av, want_q, want_qd,
            [&](int k, const T (&col)[N]) {  // -sym(H)^-1 col
                fdh_solve<T, N>(H, Di, zero, col, [&](int i, T v) { out_dq(i + N * k, gd.out(v)); });
            },
            [&](int k, const T (&col)[N]) {
                fdh_solve<T, N>(H, Di, zero, col, [&](int i, T v) { out_dqd(i + N * k, gd.out(v)); });
            });
    }
    if (want_tau) {
#pragma unroll kU
        for (int k = 0; k < N; ++k) {
            T e[N];
#pragma unroll
            for (int j = 0; j < N; ++j) e[j] = j == k ? T(1) : T(0);
            fdh_solve<T, N>(H, Di, e, zero, [&](int i, T v) { out_dtau(i + N * k, gd.out(v)); });
        }
    }
}

// Lane bodies (model-specialised kernels only, SoA rows): a NULL output is neither evaluated nor
// stored.
template <typename T, int N, bool FAST>
__device__ __forceinline__ void rnea_deriv_lane(const T *mdl, const T *__restrict__ q, const T *__restrict__ qd,
                                                const T *__restrict__ qdd, T *__restrict__ dq, T *__restrict__ dqd,
                                                uint32_t b, int64_t ld) {
    const uint32_t off = b * (uint32_t)sizeof(T);
    T qv[N], qdv[N], qddv[N];
    load_cfg<T, N>(q, qd, qdd, ld, off, qv, qdv, qddv);
    rnea_deriv_eval<T, N, FAST>(
        mdl, qv, qdv, qddv, dq != nullptr, dqd != nullptr, [&](int e, T v) { st_row(dq, e * ld, off, v); },
        [&](int e, T v) { st_row(dqd, e * ld, off, v); });
}

template <typename T, int N, bool FAST>
__device__ __forceinline__ void fd_deriv_lane(const T *mdl, const T *__restrict__ q, const T *__restrict__ qd,
                                              const T *__restrict__ tau, T *__restrict__ qdd, T *__restrict__ dq,
                                              T *__restrict__ dqd, T *__restrict__ dtau, uint32_t b, int64_t ld) {
    const uint32_t off = b * (uint32_t)sizeof(T);
    T qv[N], qdv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        qv[j] = ld_row(q, j * ld, off);
        qdv[j] = ld_row(qd, j * ld, off);
    }
    fd_deriv_eval<T, N, FAST>(
        mdl, qv, qdv,
        [&](T (&tv)[N]) {
#pragma unroll
            for (int j = 0; j < N; ++j) tv[j] = ld_row(tau, j * ld, off);
        },
        dq != nullptr, dqd != nullptr, dtau != nullptr,
        [&](int j, T v) {
            if (qdd) st_row(qdd, j * ld, off, v);
        },
        [&](int e, T v) { st_row(dq, e * ld, off, v); }, [&](int e, T v) { st_row(dqd, e * ld, off, v); },
        [&](int e, T v) { st_row(dtau, e * ld, off, v); });
}

}  // namespace dev
}  // namespace rbamd
