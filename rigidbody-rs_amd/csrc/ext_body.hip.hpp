// ext_body.hip.hpp -- inverse and forward dynamics under external link wrenches (device + host).
//
//   tau = rnea_ext(q, qd, qdd, fext) = rnea(q, qd, qdd) - sum_j J_j(q)^T fext_j
//   qdd = fd_ext(q, qd, tau, fext)   = fd(q, qd, tau + sum_j J_j(q)^T fext_j)
//
// fext_j is the spatial wrench acting ON link j, expressed in link j's own URDF link frame (the
// joint's child frame, after the joint's motion) and applied at that frame's origin; rows
// 6 j + 0..2 are the force, 6 j + 3..5 the moment ([lin; rot], the Jacobian's row order).  The
// wrench enters where the link's own force is formed (Featherstone 2008):
//   RNEA  Table 5.1   f_j  = I_j a_j + v_j x* I_j v_j - fext_j
//   ABA   Table 7.1   pA_j = v_j x* I_j v_j - fext_j
//   mass-matrix FD    C = rnea_ext(q, qd, 0, fext), then H qdd = tau - C as fdh_body.hip.hpp
// at link j's forward step, from the six rows fetched there (`fx(row)`), so the 6 n wrench values
// are never held together.  The kernels work in per-link frames whose z is the joint axis
// (model.cpp pack: x_urdf = R_a x_kernel); `ra` holds every link's R_a (9 N, row-major; jit.cpp
// emits it as compile-time constants, the host forms take Model::axis_frames()) and the wrench
// is rotated by R_a^T on arrival -- an exact identity, folded away, for z-axis links.
//
// One body per algorithm serves serial chains and trees: the recursions are tree_body.hip.hpp's
// over the `Topo` policy (compile-time parent indices and joint types), which the serial chain
// satisfies with parent(j) = j - 1 (its RNEA sweeps take rnea_body.hip.hpp's own link steps, so a
// link without a wrench contributes exactly what it does to the plain RNEA).  Every input -- the wrench rows included -- goes through the
// InputGuard; an out-of-domain configuration gets NaN in every output.
#pragma once

#include "aba_body.hip.hpp"

namespace rbamd {
namespace dev {

// Highest-index child of link j (-1: a leaf); SerialTopo does not carry it.
template <typename Topo, int N>
constexpr int ext_last_child(int j) {
    if constexpr (Topo::kSerial)
        return j + 1 < N ? j + 1 : -1;
    else
        return Topo::last_child(j);
}

// Link j's wrench in the kernel's link frame: (n, f) = (R_a^T moment, R_a^T force).
template <typename T, typename Fx>
RB_HD void ext_wrench(const T *ra, int j, Fx &&fx, InputGuard<T> &gd, V3<T> &n, V3<T> &f) {
    const V3<T> fu = v3(fx(6 * j + 0), fx(6 * j + 1), fx(6 * j + 2));
    const V3<T> nu = v3(fx(6 * j + 3), fx(6 * j + 4), fx(6 * j + 5));
    gd.val(fu.x); gd.val(fu.y); gd.val(fu.z);
    gd.val(nu.x); gd.val(nu.y); gd.val(nu.z);
    const T *r = ra + 9 * j;
    // a rotation with unit diagonal is the identity (trace 3)
    if (r[0] == T(1) && r[4] == T(1) && r[8] == T(1)) {
        f = fu;
        n = nu;
    } else {
        const M3<T> Ra{{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]}};
        f = mul_t(Ra, fu);
        n = mul_t(Ra, nu);
    }
}

// ----------------------------------------------------------------------------- RNEA
// rnea_eval_tree's sweeps with the wrench subtracted from each link force.  QDD = false: the
// bias sweep of the mass-matrix forward dynamics (qdd = 0, nothing to check or add).  Leaves
// (cos, sin) in cs / sn for a later stage and hands the raw tau_j to out(j, value), leaf first;
// the caller applies gd.
template <typename T, int N, bool FAST, typename Topo, bool QDD, typename Fx, typename Out>
RB_HD void rnea_ext_sweeps(const T *mdl, const T *ra, const T (&qv)[N], const T (&qdv)[N], const T (&qddv)[N],
                           Fx &&fx, T (&cs)[N], T (&sn)[N], InputGuard<T> &gd, Out &&out) {
    V3<T> fn[N], ff[N];  // per-link spatial force (moment, force)
    if constexpr (Topo::kSerial) {
        // The serial chain: rnea_eval's own steps (rnea_body.hip.hpp rnea_fwd0 / rnea_fwd / rnea_bwd),
        // so a link that carries no wrench contributes bit for bit what it does there.
        auto sub = [&](int j) {
            V3<T> xn, xf;
            ext_wrench(ra, j, fx, gd, xn, xf);
            fn[j] = v3(fn[j].x - xn.x, fn[j].y - xn.y, fn[j].z - xn.z);
            ff[j] = v3(ff[j].x - xf.x, ff[j].y - xf.y, ff[j].z - xf.z);
        };
        RneaState<T> st;
        rnea_fwd0<T, FAST, false, QDD>(mdl, qv[0], qdv[0], QDD ? qddv[0] : T(0), st, sn[0], cs[0], fn[0], ff[0], gd);
        sub(0);
#pragma unroll
        for (int j = 1; j < N; ++j) {
            rnea_fwd<T, FAST, false, QDD>(mdl, j, qv[j], qdv[j], QDD ? qddv[j] : T(0), st, sn[j], cs[j], fn[j], ff[j],
                                          gd);
            sub(j);
        }
        reload_fence();
#pragma unroll
        for (int j = N - 1; j >= 1; --j) {
            out(j, fn[j].z);
            rnea_bwd(mdl, j, cs[j], sn[j], ff[j], fn[j], ff[j - 1], fn[j - 1]);
        }
        out(0, fn[0].z);
    } else {
    V3<T> W[N], V[N], AW[N], AV[N];  // link velocity / acceleration (rot, lin), link coordinates
    cfor<0, N>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr int p = Topo::parent(j);
        constexpr bool pri = Topo::prismatic(j);
        const Link<T> L = load_link(mdl, j);
        const T qdj = qdv[j];
        if constexpr (pri) gd.val(qv[j]); else gd.angle(qv[j]);
        gd.val(qdj);
        if constexpr (QDD) gd.val(qddv[j]);
        if constexpr (!pri) sin_cos<FAST>(qv[j], sn[j], cs[j]); else { cs[j] = T(1); sn[j] = T(0); }
        M3<T> E;
        V3<T> r;
        link_frame<T, pri>(L, qv[j], cs[j], sn[j], E, r);
        V3<T> w, v, aw, av;
        if constexpr (p < 0) {  // base: v = 0, a = (0, (0,0,+g)) -- multibody.rs:116-120
            const T g = T(kGravity);
            w = v3(T(0), T(0), T(0));
            v = w;
            aw = w;
            av = v3(g * E.m[6], g * E.m[7], g * E.m[8]);
        } else {
            w = mul_t(E, W[p]);
            v = mul_t(E, cross_sub(V[p], r, W[p]));
            aw = mul_t(E, AW[p]);
            av = mul_t(E, cross_sub(AV[p], r, AW[p]));
        }
        if constexpr (!pri) {  // S = (e_z, 0)
            w.z += qdj;
            if constexpr (QDD) aw.z += qddv[j];
            av.x = fmadd(v.y, qdj, av.x);
            av.y = fmadd(-v.x, qdj, av.y);
            aw.x = fmadd(w.y, qdj, aw.x);
            aw.y = fmadd(-w.x, qdj, aw.y);
        } else {  // S = (0, e_z)
            v.z += qdj;
            if constexpr (QDD) av.z += qddv[j];
            av.x = fmadd(w.y, qdj, av.x);
            av.y = fmadd(-w.x, qdj, av.y);
        }
        W[j] = w;
        V[j] = v;
        AW[j] = aw;
        AV[j] = av;
        // f = I a + v x* (I v) - fext
        V3<T> n, f, xn, xf;
        link_force(L, j, w, v, aw, av, n, f);
        ext_wrench(ra, j, fx, gd, xn, xf);
        fn[j] = v3(n.x - xn.x, n.y - xn.y, n.z - xn.z);
        ff[j] = v3(f.x - xf.x, f.y - xf.y, f.z - xf.z);
    });
    reload_fence();
    cfor_rev<N>([&](auto jc) {  // tau_j = S_j^T f_j; f_parent += X_j^T f_j
        constexpr int j = decltype(jc)::value;
        constexpr int p = Topo::parent(j);
        constexpr bool pri = Topo::prismatic(j);
        out(j, pri ? ff[j].z : fn[j].z);
        if constexpr (p >= 0) {
            const Link<T> L = load_link(mdl, j);
            M3<T> E;
            V3<T> r;
            link_frame<T, pri>(L, qv[j], cs[j], sn[j], E, r);
            V3<T> n = fn[j], f = ff[j];
            force_to_parent(E, r, n, f);
            fn[p] = add3(fn[p], n);
            ff[p] = add3(ff[p], f);
        }
    });
    }  // trees
}

template <typename T, int N, bool FAST, typename Topo, typename Fx, typename Out>
RB_HD void rnea_ext_eval(const T *mdl, const T *ra, const T (&qv)[N], const T (&qdv)[N], const T (&qddv)[N], Fx &&fx,
                         Out &&out) {
    InputGuard<T> gd;
    T cs[N], sn[N];
    rnea_ext_sweeps<T, N, FAST, Topo, true>(mdl, ra, qv, qdv, qddv, static_cast<Fx &&>(fx), cs, sn, gd,
                                            [&](int j, T v) { out(j, gd.out(v)); });
}

// ---------------------------------------------------------- mass-matrix forward dynamics
// fdh_eval / fdh_eval_tree with the bias C = rnea_ext(q, qd, 0, fext); tau is loaded after the
// bias sweep, as there.
template <typename T, int N, bool FAST, typename Topo, typename Fx, typename Tau, typename Out>
RB_HD void fdh_ext_eval(const T *mdl, const T *ra, const T (&qv)[N], const T (&qdv)[N], Fx &&fx, Tau &&load_tau,
                        Out &&out) {
    T cs[N], sn[N], C[N], tv[N], H[N][N], Di[N];
    InputGuard<T> gd;
    rnea_ext_sweeps<T, N, FAST, Topo, false>(mdl, ra, qv, qdv, qdv /* unread */, static_cast<Fx &&>(fx), cs, sn, gd,
                                             [&](int j, T v) { C[j] = v; });
    load_tau(tv);
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
    fdh_solve<T, N>(H, Di, tv, C, [&](int j, T v) { out(j, gd.out(v)); });
}

// ------------------------------------------------------------------------------ ABA
// aba_eval_tree with pA_j = v_j x* I_j v_j - fext_j.
template <typename T, int N, bool FAST, typename Topo, typename Fx, typename Out>
RB_HD void aba_ext_eval(const T *mdl, const T *ra, const T (&qv)[N], const T (&qdv)[N], const T (&tv)[N], Fx &&fx,
                        Out &&out_) {
    InputGuard<T> gd;
    gd.vals(tv);
    auto out = [&](int j, T v) { out_(j, gd.out(v)); };
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
    V3<T> UrD[N], UlD[N];  // U / D (its S-component is exactly 1)
    T uD[N];
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
        V3<T> ur, ul;
        T D, u;
        if constexpr (!pri) {
            ur = v3(IA.A.xz, IA.A.yz, IA.A.zz);
            ul = v3(IA.B.m[6], IA.B.m[7], IA.B.m[8]);
            D = IA.A.zz;
            u = tv[j] - An.z;
        } else {
            ur = v3(IA.B.m[2], IA.B.m[5], IA.B.m[8]);
            ul = v3(IA.M.xz, IA.M.yz, IA.M.zz);
            D = IA.M.zz;
            u = tv[j] - Af.z;
        }
        const T Dinv = recip(D);
        V3<T> dr = v3(ur.x * Dinv, ur.y * Dinv, ur.z * Dinv);
        V3<T> dl = v3(ul.x * Dinv, ul.y * Dinv, ul.z * Dinv);
        if constexpr (!pri) dr.z = T(1); else dl.z = T(1);
        UrD[j] = dr;
        UlD[j] = dl;
        uD[j] = u * Dinv;
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
            M3<T> E;
            V3<T> r;
            link_frame<T, pri>(L, qv[j], cs[j], sn[j], E, r);
            force_to_parent(E, r, pa_n, pa_f);
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
        }
    });

    reload_fence();
    V3<T> AW[N], AV[N];
    cfor<0, N>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr int p = Topo::parent(j);
        constexpr bool pri = Topo::prismatic(j);
        const Link<T> L = load_link(mdl, j);
        M3<T> E;
        V3<T> r;
        link_frame<T, pri>(L, qv[j], cs[j], sn[j], E, r);
        V3<T> aw, av;
        if constexpr (p < 0) {
            const T g = T(kGravity);
            aw = v3(T(0), T(0), T(0));
            av = v3(g * E.m[6], g * E.m[7], g * E.m[8]);
        } else {
            aw = mul_t(E, AW[p]);
            av = mul_t(E, cross_sub(AV[p], r, AW[p]));
        }
        aw.x += cw0[j]; aw.y += cw1[j];
        av.x += cv0[j]; av.y += cv1[j];
        const V3<T> dr = UrD[j], dl = UlD[j];
        const T a = uD[j] - fmadd(dr.x, aw.x, fmadd(dr.y, aw.y, fmadd(dr.z, aw.z,
                                  fmadd(dl.x, av.x, fmadd(dl.y, av.y, dl.z * av.z)))));
        if constexpr (!pri) aw.z += a; else av.z += a;
        AW[j] = aw;
        AV[j] = av;
        out(j, a);
    });
}

// ---------------------------------------------------------------------- lane bodies
// One configuration per lane on SoA rows.  q, qd (and qdd / the ABA's tau) are loaded up front in
// first-use order as in the neighbouring lane bodies; the wrench rows are loaded by the link
// step that consumes them, under the same RB_NT policy (every element is read once).
template <typename T, int N, bool FAST, typename Topo = SerialTopo>
__device__ __forceinline__ void rnea_ext_lane(const T *mdl, const T *ra, const T *__restrict__ q,
                                              const T *__restrict__ qd, const T *__restrict__ qdd,
                                              const T *__restrict__ fext, T *__restrict__ tau, uint32_t b,
                                              int64_t ld) {
    const uint32_t off = b * (uint32_t)sizeof(T);
    T qv[N], qdv[N], qddv[N];
    load_cfg<T, N>(q, qd, qdd, ld, off, qv, qdv, qddv);
    rnea_ext_eval<T, N, FAST, Topo>(
        mdl, ra, qv, qdv, qddv, [&](int r) { return ld_row(fext, r * ld, off); },
        [&](int j, T v) { st_row(tau, j * ld, off, v); });
}

// FDH: the mass-matrix form (jit_fd_form 2), else the ABA.
template <typename T, int N, bool FAST, typename Topo, bool FDH>
__device__ __forceinline__ void fd_ext_lane(const T *mdl, const T *ra, const T *__restrict__ q,
                                            const T *__restrict__ qd, const T *__restrict__ tau,
                                            const T *__restrict__ fext, T *__restrict__ qdd, uint32_t b,
                                            int64_t ld) {
    const uint32_t off = b * (uint32_t)sizeof(T);
    T qv[N], qdv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        qv[j] = ld_row(q, j * ld, off);
        __builtin_amdgcn_sched_barrier(0);
        qdv[j] = ld_row(qd, j * ld, off);
        __builtin_amdgcn_sched_barrier(0);
    }
    auto fx = [&](int r) { return ld_row(fext, r * ld, off); };
    auto store = [&](int j, T v) { st_row(qdd, j * ld, off, v); };
    if constexpr (FDH) {
        fdh_ext_eval<T, N, FAST, Topo>(mdl, ra, qv, qdv, fx,
                                       [&](T (&tv)[N]) {
#pragma unroll
                                           for (int j = 0; j < N; ++j) {
                                               tv[j] = ld_row(tau, j * ld, off);
                                               __builtin_amdgcn_sched_barrier(0);
                                           }
                                       },
                                       store);
    } else {
        T tv[N];
#pragma unroll
        for (int j = N - 1; j >= 0; --j) {
            tv[j] = ld_row(tau, j * ld, off);
            __builtin_amdgcn_sched_barrier(0);
        }
        aba_ext_eval<T, N, FAST, Topo>(mdl, ra, qv, qdv, tv, fx, store);
    }
}

}  // namespace dev
}  // namespace rbamd
