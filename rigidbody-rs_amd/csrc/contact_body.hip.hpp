// contact_body.hip.hpp -- compliant ground contact (device + host).
//
//   contact_wrench(q, qd)            -> fext, cforce   the contact set's wrench on every link
//   rollout_contact(q, qd, tau_seq)  -> traj           K semi-implicit Euler steps of fd_ext under it
//
// A contact set is model data (model.hpp ContactSet): P points, each fixed to a moving link l_p at
// c_p in that link's URDF link frame; one plane in the base frame (unit normal nhat, offset d, the
// free side nhat . x > d); stiffness k, damping c, friction mu, slip velocity v_s.  With pos_j, R_j
// and vel_j = [lin_j; ang_j] as link_kin_body.hip.hpp defines them:
//
//   x_p   = pos_l + R_l c_p                          point in the base frame
//   xd_p  = R_l (lin_l + ang_l x c_p)                its velocity in the base frame
//   phi   = max(d - nhat . x_p, 0)                   penetration depth
//   phid  = -nhat . xd_p                             penetration rate
//   f_n   = max(k * phi * (1 + c * phid), 0)         Hunt-Crossley normal force, never adhesive
//   v_t   = xd_p + phid * nhat                       tangential velocity
//   F_p   = f_n * nhat - mu * f_n * v_t / sqrt(v_t . v_t + v_s^2)
//   g_p   = R_l^T F_p                                the force in the link frame
//   fext_l += [ g_p ; c_p x g_p ]                    [force; moment], fext's row order
//
// Every piece is continuous in the state.  cforce [3 P] holds F_p (base frame), row 3 p + c.
//
// One root-to-leaf sweep carries a link's world pose and its velocity together -- link_kin_body's two
// sweeps merged, one sincos per joint, the same "keep only branch links" slots.  The sweep runs in
// the kernels' per-link frames (x_urdf = R_a x_kernel); only a link that carries a point turns
// anything: c_p into the kernel frame on the way in (constants), its summed wrench into the URDF
// frame on the way out.  The wrench of the links that carry points is all a lane holds: `fw`,
// Con::kSlots x 6 values, which the dynamics then read through their `fx(row)` hook
// (ext_body.hip.hpp) -- a link without a point reads the literal 0.
//
// `Con` describes the set: on the device a struct of compile-time constants (jit.cpp emits it, so
// mu == 0 folds the friction away, and a changed stiffness is a different kernel), on the host a
// view of the model's ContactSet.  kSlots bounds the links that carry points; slot_of(j) is link
// j's row of fw (-1: no point).
//
// The lane bodies check every input before the first store (InputGuard); fp32 outputs leave through
// lk_out (link_kin_body.hip.hpp): a value can be a product whose constant factors fold to +-1, that
// is a raw transcendental result (a rotation entry, a hardware sin / cos), which the guard's inline
// assembly must not read without a wait state.
#pragma once

#include "ext_body.hip.hpp"
#include "link_kin_body.hip.hpp"

namespace rbamd {
namespace dev {

// Con's bounds are compile-time constants on the device only: the host's loops stay loops.
#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC_RTC__)
#define RB_CT_UNROLL _Pragma("unroll")
#else
#define RB_CT_UNROLL
#endif

RB_HD float ct_sqrt(float x) { return __builtin_sqrtf(x); }
RB_HD double ct_sqrt(double x) { return __builtin_sqrt(x); }

// A value the dynamics' guard will read through inline assembly: the same one-instruction wait
// lk_out puts in front of it (fp32 on the device only).
template <typename T>
RB_HD T ct_settle(T v) {
#if RB_GUARD_ASM
    if constexpr (!__is_same(T, double)) asm("s_nop 1 ; rb_settle" : "+v"(v));
#endif
    return v;
}

// The contact law at one point: position x and velocity xd in the base frame -> F.  Returns f_n.
template <typename T, typename Con>
RB_HD T contact_law(const Con &con, const V3<T> &x, const V3<T> &xd, V3<T> &F) {
    const V3<T> nh = v3(con.normal(0), con.normal(1), con.normal(2));
    const T gap = con.offset() - fmadd(nh.x, x.x, fmadd(nh.y, x.y, nh.z * x.z));
    const T phi = gap > T(0) ? gap : T(0);
    const T phid = -fmadd(nh.x, xd.x, fmadd(nh.y, xd.y, nh.z * xd.z));
    const T hc = con.stiffness() * phi * fmadd(con.damping(), phid, T(1));
    const T fn = hc > T(0) ? hc : T(0);
    F = v3(fn * nh.x, fn * nh.y, fn * nh.z);
    if (con.friction() != T(0)) {
        const V3<T> vt = v3(fmadd(phid, nh.x, xd.x), fmadd(phid, nh.y, xd.y), fmadd(phid, nh.z, xd.z));
        const T vs = con.slip_velocity();
        const T den = ct_sqrt(fmadd(vt.x, vt.x, fmadd(vt.y, vt.y, fmadd(vt.z, vt.z, vs * vs))));  // >= v_s
        const T s = con.friction() * fn / den;
        F = v3(fmadd(-s, vt.x, F.x), fmadd(-s, vt.y, F.y), fmadd(-s, vt.z, F.z));
    }
    return fn;
}

// fw[s][0..2] the force, fw[s][3..5] the moment on the link of slot s, in its URDF link frame;
// out_c(row, value) over 3 P rows as each point completes.  Values are raw: the caller guards.
template <typename T, int N, bool FAST, typename Topo, typename Con, typename OutC>
RB_HD void contact_eval(const T *mdl, const T *ra, const Con &con, const T (&qv)[N], const T (&qdv)[N],
                        T (&fw)[Con::kSlots][6], OutC &&out_c) {
    LkPose<T> cur, kept[lk_slots<Topo, N>()];
    LkVel<T> vcur, vkept[lk_slots<Topo, N>()];
    cfor<0, N>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr int p = Topo::parent(j);
        constexpr bool pri = Topo::prismatic(j);
        const Link<T> L = load_link(mdl, j);
        T c = T(1), s = T(0);
        if constexpr (!pri) sin_cos<FAST>(qv[j], s, c);
        M3<T> E;
        V3<T> r;
        link_frame<T, pri>(L, qv[j], c, s, E, r);
        LkPose<T> X;
        LkVel<T> U;
        if constexpr (p < 0) {  // a root link: its frame in the base, the base at rest
            X.R = E;
            X.p = r;
            U.w = v3(T(0), T(0), T(0));
            U.v = U.w;
        } else {
            LkPose<T> P;
            LkVel<T> Q;
            if constexpr (p == j - 1) {
                P = cur;
                Q = vcur;
            } else {
                P = kept[lk_slot<Topo, N>(p)];
                Q = vkept[lk_slot<Topo, N>(p)];
            }
            X.p = mul_add(P.p, P.R, r);
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    X.R.m[3 * a + b] = fmadd(P.R.m[3 * a + 0], E.m[b],
                                             fmadd(P.R.m[3 * a + 1], E.m[3 + b], P.R.m[3 * a + 2] * E.m[6 + b]));
            U.w = mul_t(E, Q.w);
            U.v = mul_t(E, cross_sub(Q.v, r, Q.w));
        }
        if constexpr (!pri) U.w.z += qdv[j]; else U.v.z += qdv[j];  // S = (e_z, 0) / (0, e_z)
        cur = X;
        vcur = U;
        if constexpr (lk_branch<Topo, N>(j)) {
            kept[lk_slot<Topo, N>(j)] = X;
            vkept[lk_slot<Topo, N>(j)] = U;
        }
        const int slot = con.slot_of(j);
        if (slot >= 0) {  // this link carries points: the only place the URDF frame enters
            const T *A = ra + 9 * j;
            const M3<T> Ra{{A[0], A[1], A[2], A[3], A[4], A[5], A[6], A[7], A[8]}};
            const bool turn = !lk_identity(A);
            V3<T> gf = v3(T(0), T(0), T(0)), gm = gf;  // summed force / moment, kernel frame
            RB_CT_UNROLL
            for (int k = 0; k < con.points(); ++k) {
                if (con.link(k) != j) continue;
                V3<T> ck = v3(con.point(k, 0), con.point(k, 1), con.point(k, 2));
                if (turn) ck = mul_t(Ra, ck);  // x_kernel = R_a^T x_urdf
                const V3<T> x = mul_add(X.p, X.R, ck);
                const V3<T> xd = mul(X.R, cross_add(U.v, U.w, ck));
                V3<T> F;
                contact_law(con, x, xd, F);
                out_c(3 * k + 0, F.x);
                out_c(3 * k + 1, F.y);
                out_c(3 * k + 2, F.z);
                const V3<T> g = mul_t(X.R, F);
                gf = add3(gf, g);
                gm = cross_add(gm, ck, g);
            }
            if (turn) {
                gf = mul(Ra, gf);
                gm = mul(Ra, gm);
            }
            fw[slot][0] = gf.x; fw[slot][1] = gf.y; fw[slot][2] = gf.z;
            fw[slot][3] = gm.x; fw[slot][4] = gm.y; fw[slot][5] = gm.z;
        }
    });
}

// The whole [6 N] wrench and [3 P] point forces of one configuration through its guard:
// out_f(row, value) link by link (exact zeros for links without a point), out_c as above.
template <typename T, int N, bool FAST, typename Topo, typename Con, typename OutF, typename OutC>
RB_HD void contact_wrench_eval(const T *mdl, const T *ra, const Con &con, const T (&qv)[N], const T (&qdv)[N],
                               OutF &&out_f, OutC &&out_c) {
    InputGuard<T> gd;
    gd.template joints<Topo>(qv);
    gd.vals(qdv);
    T fw[Con::kSlots][6];
    contact_eval<T, N, FAST, Topo>(mdl, ra, con, qv, qdv, fw, [&](int e, T v) { out_c(e, lk_out(gd, v)); });
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int slot = con.slot_of(j);
#pragma unroll
        for (int e = 0; e < 6; ++e) out_f(6 * j + e, lk_out(gd, slot >= 0 ? fw[slot][e] : T(0)));
    }
}

// One step's forward dynamics under the contact set: the wrench, then fd_ext with an fx that reads
// it (FDH: the mass-matrix form, else the ABA; both check q, qd, tau and the wrench).  The contact
// sweep and the dynamics each evaluate their own sincos.
template <typename T, int N, bool FAST, typename Topo, bool FDH, typename Con, typename Tau, typename Out>
RB_HD void contact_fd(const T *mdl, const T *ra, const Con &con, const T (&qv)[N], const T (&qdv)[N], Tau &&load_tau,
                      Out &&out) {
    T fw[Con::kSlots][6];
    contact_eval<T, N, FAST, Topo>(mdl, ra, con, qv, qdv, fw, [](int, T) {});
    auto fx = [&](int r) {
        const int slot = con.slot_of(r / 6);
        return slot >= 0 ? ct_settle(fw[slot][r % 6]) : T(0);
    };
    if constexpr (FDH) {
        fdh_ext_eval<T, N, FAST, Topo>(mdl, ra, qv, qdv, fx, static_cast<Tau &&>(load_tau), static_cast<Out &&>(out));
    } else {
        T tv[N];
        load_tau(tv);
        aba_ext_eval<T, N, FAST, Topo>(mdl, ra, qv, qdv, tv, fx, static_cast<Out &&>(out));
    }
}

// K steps on one configuration held in qv / qdv (the host form, and the register-state lane):
//   a = fd_ext(q, v, tau_k, contact(q, v));  v += dt a;  q += dt v;  traj_k = q
template <typename T, int N, bool FAST, typename Topo, bool FDH, typename Con, typename Tau, typename Traj>
RB_HD void rollout_contact_steps(const T *mdl, const T *ra, const Con &con, T (&qv)[N], T (&qdv)[N], T dt, int K,
                                 Tau &&load_tau, Traj &&traj) {
    for (int k = 0; k < K; ++k) {
        T a[N];
        contact_fd<T, N, FAST, Topo, FDH>(mdl, ra, con, qv, qdv, [&](T (&tv)[N]) { load_tau(k, tv); },
                                          [&](int j, T v) { a[j] = v; });
#pragma unroll
        for (int j = 0; j < N; ++j) {
            qdv[j] = fmadd(dt, a[j], qdv[j]);
            qv[j] = fmadd(dt, qdv[j], qv[j]);
        }
#pragma unroll
        for (int j = 0; j < N; ++j) traj(k, j, qv[j]);
    }
}

// ---------------------------------------------------------------------- lane bodies
// One configuration per lane on SoA rows: fext [6 N][ld], cforce [3 P][ld].
template <typename T, int N, bool FAST, typename Topo, typename Con>
__device__ __forceinline__ void contact_wrench_lane(const T *mdl, const T *ra, const T *__restrict__ q,
                                                    const T *__restrict__ qd, T *__restrict__ fext,
                                                    T *__restrict__ cforce, uint32_t b, int64_t ld) {
    const uint32_t off = b * (uint32_t)sizeof(T);
    T qv[N], qdv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        qv[j] = ld_row(q, j * ld, off);
        qdv[j] = ld_row(qd, j * ld, off);
    }
    contact_wrench_eval<T, N, FAST, Topo>(
        mdl, ra, Con{}, qv, qdv, [&](int e, T v) { st_row(fext, e * ld, off, v); },
        [&](int e, T v) { st_row(cforce, e * ld, off, v); });
}

// rollout_lane (aba_body.hip.hpp) with the contact step: the state in LDS between steps where
// rollout_lds_state allows, in registers otherwise; traj is required.
template <typename T, int N, bool FAST, typename Topo, bool FDH, typename Con>
__device__ __forceinline__ void rollout_contact_lane(const T *mdl, const T *ra, T *__restrict__ q, T *__restrict__ qd,
                                                     const T *__restrict__ tau_seq, T dt, int K, T *__restrict__ traj,
                                                     uint32_t b, int64_t ld, RolloutShared<T, N> &sh) {
    const uint32_t off = b * (uint32_t)sizeof(T);
    if constexpr (rollout_lds_state<T, N>()) {
        T *sx = sh.x + threadIdx.x;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            sx[j * kRolloutBlock] = ld_row(q, j * ld, off);
            sx[(N + j) * kRolloutBlock] = ld_row(qd, j * ld, off);
        }
        for (int k = 0; k < K; ++k) {
            T qv[N], qdv[N];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                qv[j] = sx[j * kRolloutBlock];
                qdv[j] = sx[(N + j) * kRolloutBlock];
            }
            auto load_tau = [&](T (&tv)[N]) {
#pragma unroll
                for (int j = 0; j < N; ++j) tv[j] = ld_row(tau_seq, ((int64_t)k * N + j) * ld, off);
            };
            contact_fd<T, N, FAST, Topo, FDH>(mdl, ra, Con{}, qv, qdv, load_tau, [&](int j, T a) {
                const T qdn = fmadd(dt, a, sx[(N + j) * kRolloutBlock]);
                const T qn = fmadd(dt, qdn, sx[j * kRolloutBlock]);
                sx[(N + j) * kRolloutBlock] = qdn;
                sx[j * kRolloutBlock] = qn;
                st_row(traj, ((int64_t)k * N + j) * ld, off, qn);
            });
        }
#pragma unroll
        for (int j = 0; j < N; ++j) {
            st_row(q, j * ld, off, sx[j * kRolloutBlock]);
            st_row(qd, j * ld, off, sx[(N + j) * kRolloutBlock]);
        }
    } else {
        T qv[N], qdv[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            qv[j] = ld_row(q, j * ld, off);
            qdv[j] = ld_row(qd, j * ld, off);
        }
        rollout_contact_steps<T, N, FAST, Topo, FDH>(
            mdl, ra, Con{}, qv, qdv, dt, K,
            [&](int k, T (&tv)[N]) {
#pragma unroll
                for (int j = 0; j < N; ++j) tv[j] = ld_row(tau_seq, ((int64_t)k * N + j) * ld, off);
            },
            [&](int k, int j, T v) { st_row(traj, ((int64_t)k * N + j) * ld, off, v); });
        uint32_t off2 = off;  // row addresses re-derived after the loop, as rollout_lane
        asm volatile("" : "+v"(off2));
#pragma unroll
        for (int j = 0; j < N; ++j) {
            st_row(q, j * ld, off2, qv[j]);
            st_row(qd, j * ld, off2, qdv[j]);
        }
    }
}

}  // namespace dev
}  // namespace rbamd
