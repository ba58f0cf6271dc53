// rnea_vjp_body.hip.hpp -- reverse-mode gradient of the inverse dynamics (device + host).
//
//   tau = rnea_ext(q, qd, qdd, fext)     (ext_body.hip.hpp; EXT = false: the plain RNEA)
//   L   = sum_i w_i tau_i                (w: the cotangent of tau)
//   g_q = dL/dq, g_qd = dL/dqd, g_qdd = dL/dqdd = sym(H) w, g_fext_j = dL/dfext_j = -J_j w
//
// One O(n) reverse sweep of the RNEA over the `Topo` policy (tree_body.hip.hpp: compile-time parent
// indices and joint types), one configuration per lane; no Jacobian or n x n matrix is formed.
// Spatial vectors are (rot, lin) pairs in the kernels' per-link frames whose z is the joint axis,
// S = (e_z, 0) for a revolute joint and (0, e_z) for a prismatic one; `ra` holds every link's R_a
// (x_urdf = R_a x_kernel) to turn the wrench rows in and the g_fext rows out, as ext_body.hip.hpp
// and link_kin_body.hip.hpp do.  x is the motion cross product, x* the force one.
//
// Pass A, root to leaf, is the RNEA's forward sweep
//   v_j = X_j v_p + S qd_j,  a_j = X_j a_p + S qdd_j + v_j x S qd_j,  f_j = I_j a_j + v_j x* I_j v_j - e_j
// fused with the adjoint of the transmitted force F_j, a motion vector:
//   phi_j = X_j phi_p + S w_j        (phi_base = 0: link_vel(q, w), so g_fext_j = -phi_j)
// because L = sum_j phi_j . f_j.  It keeps per link v_j, phi_j, f_j, (cos, sin) and the four nonzero
// components of S x (X_j a_p) = S x (a_j - v_j x S qd_j).
//
// Pass B, leaf to root, accumulates three force-type vectors, each handed to the parent as X_j^T . :
//   F_j = f_j + sum_c X_c^T F_c                                        (the RNEA's backward sweep)
//   A_j = I_j phi_j + sum_c X_c^T A_c                                  (adjoint of a_j)
//   V_j = -phi_j x* h_j - I_j (v_j x phi_j) + qd_j (S x* A_j) + sum_c X_c^T V_c,  h_j = I_j v_j
// and reads the gradient off them (dX_j/dq_j u = -S x (X_j u)):
//   g_qdd_j = S . A_j
//   g_qd_j  = S . V_j + A_j . (v_j x S)
//   g_q_j   = phi_j . (S x* F_j) - A_j . (S x (a_j - v_j x S qd_j)) - V_j . (S x v_j)
// A prismatic joint changes S only; a root link takes X_j a_base for X_j a_p.
//
// Every input -- the wrench rows included -- goes through the InputGuard before the first store: the
// wrench rows are fetched link by link in pass A, so every output, g_fext too, leaves in pass B.
// The cotangent w is not checked: a NaN there propagates by arithmetic.
#pragma once

#include "ext_body.hip.hpp"
#include "link_kin_body.hip.hpp"

namespace rbamd {
namespace dev {

// (add3's sibling; it lives here and not beside add3 in tree_body.hip.hpp so that no shared header -- and so
// no existing kernel's compiled source -- changes with this file)
template <typename T>
RB_HD V3<T> sub3(const V3<T> &a, const V3<T> &b) {
    return v3(a.x - b.x, a.y - b.y, a.z - b.z);
}

// fx(row): wrench row of this configuration (EXT only).  want_f: g_fext is asked for.
// out_q / out_qd / out_qdd (j, value) over N rows, out_f(row, value) over 6 N rows, leaf first.
template <typename T, int N, bool FAST, typename Topo, bool EXT, typename Fx, typename OQ, typename OQd, typename OQdd,
          typename OF>
RB_HD void rnea_vjp_eval(const T *mdl, const T *ra, const T (&qv)[N], const T (&qdv)[N], const T (&qddv)[N],
                         const T (&wv)[N], Fx &&fx, bool want_f, OQ &&out_q, OQd &&out_qd, OQdd &&out_qdd,
                         OF &&out_f) {
    InputGuard<T> gd;
    T cs[N], sn[N];
    V3<T> W[N], V[N], AW[N], AV[N];  // link velocity / acceleration (rot, lin), link coordinates
    V3<T> PW[N], PV[N];              // phi_j (rot, lin)
    V3<T> fn[N], ff[N];              // f_j, then F_j (moment, force)
    T k0[N], k1[N], k2[N], k3[N];    // S x (X_j a_p): rot x, y and lin x, y
    cfor<0, N>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr int p = Topo::parent(j);
        constexpr bool pri = Topo::prismatic(j);
        const Link<T> L = load_link(mdl, j);
        const T qdj = qdv[j];
        if constexpr (pri) gd.val(qv[j]); else gd.angle(qv[j]);
        gd.val(qdj);
        gd.val(qddv[j]);
        if constexpr (!pri) sin_cos<FAST>(qv[j], sn[j], cs[j]); else { cs[j] = T(1); sn[j] = T(0); }
        M3<T> E;
        V3<T> r;
        link_frame<T, pri>(L, qv[j], cs[j], sn[j], E, r);
        V3<T> w, v, aw, av, pw, pv;
        if constexpr (p < 0) {  // base: v = 0, a = (0, (0,0,+g)), phi = 0
            const T g = T(kGravity);
            w = v3(T(0), T(0), T(0));
            v = w;
            aw = w;
            av = v3(g * E.m[6], g * E.m[7], g * E.m[8]);
            pw = w;
            pv = w;
        } else {
            w = mul_t(E, W[p]);
            v = mul_t(E, cross_sub(V[p], r, W[p]));
            aw = mul_t(E, AW[p]);
            av = mul_t(E, cross_sub(AV[p], r, AW[p]));
            pw = mul_t(E, PW[p]);
            pv = mul_t(E, cross_sub(PV[p], r, PW[p]));
        }
        if constexpr (!pri) {  // S = (e_z, 0): S x c = (e_z x c_rot, e_z x c_lin)
            k0[j] = -aw.y; k1[j] = aw.x;
            k2[j] = -av.y; k3[j] = av.x;
            w.z += qdj;
            aw.z += qddv[j];
            av.x = fmadd(v.y, qdj, av.x);
            av.y = fmadd(-v.x, qdj, av.y);
            aw.x = fmadd(w.y, qdj, aw.x);
            aw.y = fmadd(-w.x, qdj, aw.y);
            pw.z += wv[j];
        } else {  // S = (0, e_z): S x c = (0, e_z x c_rot)
            k0[j] = T(0); k1[j] = T(0);
            k2[j] = -aw.y; k3[j] = aw.x;
            v.z += qdj;
            av.z += qddv[j];
            av.x = fmadd(w.y, qdj, av.x);
            av.y = fmadd(-w.x, qdj, av.y);
            pv.z += wv[j];
        }
        W[j] = w;
        V[j] = v;
        AW[j] = aw;
        AV[j] = av;
        PW[j] = pw;
        PV[j] = pv;
        // f = I a + v x* (I v) - fext
        V3<T> n, f;
        link_force(L, j, w, v, aw, av, n, f);
        if constexpr (EXT) {
            V3<T> xn, xf;
            ext_wrench(ra, j, fx, gd, xn, xf);
            n = sub3(n, xn);
            f = sub3(f, xf);
        }
        fn[j] = n;
        ff[j] = f;
    });
    reload_fence();
    V3<T> An[N], Af[N], Vn[N], Vf[N];  // what the children have handed up so far
#pragma unroll
    for (int j = 0; j < N; ++j) {
        An[j] = v3(T(0), T(0), T(0));
        Af[j] = An[j];
        Vn[j] = An[j];
        Vf[j] = An[j];
    }
    cfor_rev<N>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr int p = Topo::parent(j);
        constexpr bool pri = Topo::prismatic(j);
        const Link<T> L = load_link(mdl, j);
        const V3<T> w = W[j], v = V[j], pw = PW[j], pv = PV[j];
        const T qdj = qdv[j];
        // A = I phi + children
        V3<T> an, af;
        inertia_mul(L, pw, pv, an, af);
        an = add3(an, An[j]);
        af = add3(af, Af[j]);
        // V = -phi x* h - I (v x phi) + qd (S x* A) + children,  h = I v
        V3<T> hn, hf, un, uf;
        inertia_mul(L, w, v, hn, hf);
        inertia_mul(L, cross(w, pw), cross_add(cross(w, pv), v, pw), un, uf);
        V3<T> vn = sub3(cross_sub(cross_sub(Vn[j], pw, hn), pv, hf), un);
        V3<T> vf = sub3(cross_sub(Vf[j], pw, hf), uf);
        if constexpr (!pri) {  // S x* A = (e_z x A_n, e_z x A_f)
            vn.x = fmadd(-an.y, qdj, vn.x);
            vn.y = fmadd(an.x, qdj, vn.y);
            vf.x = fmadd(-af.y, qdj, vf.x);
            vf.y = fmadd(af.x, qdj, vf.y);
        } else {  // S x* A = (e_z x A_f, 0)
            vn.x = fmadd(-af.y, qdj, vn.x);
            vn.y = fmadd(af.x, qdj, vn.y);
        }
        const V3<T> Fn = fn[j], Ff = ff[j];
        T gq, gqd, gqdd;
        if constexpr (!pri) {
            gqdd = an.z;
            // S . V + A . (v x S),  x x e_z = (x.y, -x.x, 0)
            gqd = fmadd(an.x, w.y, fmadd(-an.y, w.x, fmadd(af.x, v.y, fmadd(-af.y, v.x, vn.z))));
            // phi . (S x* F) - A . K - V . (S x v),  e_z x x = (-x.y, x.x, 0)
            const T t0 = fmadd(pw.y, Fn.x, fmadd(-pw.x, Fn.y, fmadd(pv.y, Ff.x, -pv.x * Ff.y)));
            const T t1 = fmadd(an.x, k0[j], fmadd(an.y, k1[j], fmadd(af.x, k2[j], af.y * k3[j])));
            const T t2 = fmadd(vn.y, w.x, fmadd(-vn.x, w.y, fmadd(vf.y, v.x, -vf.x * v.y)));
            gq = t0 - t1 - t2;
        } else {
            gqdd = af.z;
            gqd = fmadd(af.x, w.y, fmadd(-af.y, w.x, vf.z));
            const T t0 = fmadd(pw.y, Ff.x, -pw.x * Ff.y);
            const T t1 = fmadd(af.x, k2[j], af.y * k3[j]);
            const T t2 = fmadd(vf.y, w.x, -vf.x * w.y);
            gq = t0 - t1 - t2;
        }
        out_q(j, lk_out(gd, gq));
        out_qd(j, lk_out(gd, gqd));
        out_qdd(j, lk_out(gd, gqdd));
        if constexpr (EXT) {
            if (want_f) {  // g_fext_j = -R_a phi_j, rows [lin; rot]
                const T *A = ra + 9 * j;
                V3<T> lin = pv, ang = pw;
                if (!lk_identity(A)) {
                    const M3<T> Ra{{A[0], A[1], A[2], A[3], A[4], A[5], A[6], A[7], A[8]}};
                    lin = mul(Ra, pv);
                    ang = mul(Ra, pw);
                }
                out_f(6 * j + 0, lk_out(gd, -lin.x));
                out_f(6 * j + 1, lk_out(gd, -lin.y));
                out_f(6 * j + 2, lk_out(gd, -lin.z));
                out_f(6 * j + 3, lk_out(gd, -ang.x));
                out_f(6 * j + 4, lk_out(gd, -ang.y));
                out_f(6 * j + 5, lk_out(gd, -ang.z));
            }
        }
        if constexpr (p >= 0) {
            M3<T> E;
            V3<T> r;
            link_frame<T, pri>(L, qv[j], cs[j], sn[j], E, r);
            V3<T> n = Fn, f = Ff;
            force_to_parent(E, r, n, f);
            fn[p] = add3(fn[p], n);
            ff[p] = add3(ff[p], f);
            force_to_parent(E, r, an, af);
            An[p] = add3(An[p], an);
            Af[p] = add3(Af[p], af);
            force_to_parent(E, r, vn, vf);
            Vn[p] = add3(Vn[p], vn);
            Vf[p] = add3(Vf[p], vf);
        }
    });
}

// ---------------------------------------------------------------------- lane body
// One configuration per lane on SoA rows.  q, qd, qdd and w are loaded up front; the wrench rows
// by the link step that consumes them (EXT only), under the same RB_NT policy as the neighbouring
// one-per-lane kernels (every element is read once).  EXT = false never touches fext / g_fext.
template <typename T, int N, bool FAST, typename Topo, bool EXT>
__device__ __forceinline__ void rnea_vjp_lane(const T *mdl, const T *ra, const T *__restrict__ q,
                                              const T *__restrict__ qd, const T *__restrict__ qdd,
                                              const T *__restrict__ fext, const T *__restrict__ w,
                                              T *__restrict__ g_q, T *__restrict__ g_qd, T *__restrict__ g_qdd,
                                              T *__restrict__ g_fext, uint32_t b, int64_t ld) {
    const uint32_t off = b * (uint32_t)sizeof(T);
    T qv[N], qdv[N], qddv[N], wv[N];
    load_cfg<T, N>(q, qd, qdd, ld, off, qv, qdv, qddv);
#pragma unroll
    for (int j = 0; j < N; ++j) wv[j] = ld_row(w, j * ld, off);
    rnea_vjp_eval<T, N, FAST, Topo, EXT>(
        mdl, ra, qv, qdv, qddv, wv, [&](int r) { return ld_row(fext, r * ld, off); }, EXT,
        [&](int j, T v) { st_row(g_q, j * ld, off, v); }, [&](int j, T v) { st_row(g_qd, j * ld, off, v); },
        [&](int j, T v) { st_row(g_qdd, j * ld, off, v); }, [&](int r, T v) { st_row(g_fext, r * ld, off, v); });
}

}  // namespace dev
}  // namespace rbamd
