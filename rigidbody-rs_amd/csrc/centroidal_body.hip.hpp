// centroidal_body.hip.hpp -- whole-body quantities (device + host).
//
//   com(q)             -> com [3]                 centre of mass, base frame
//   centroidal(q, qd)  -> com [3], hg [6], energy [2]
//                         hg = [l; k]: linear momentum and angular momentum about com, base axes
//                         ([lin; ang], the ABI's row order); energy = (T, U), U = g M com_z
//   cmm(q)             -> ag [6 N]                 the centroidal momentum matrix A_G, hg = A_G qd,
//                         element row + 6 col (the Jacobian's order); rows 0..2 / M: the COM Jacobian
//
// With pos_j, R_j, lin_j, ang_j of link_kin_body.hip.hpp and m_j, c_j, Ic_j link j's mass, centre of
// mass and rotational inertia about it (include/rigidbody_batch.h has the definitions in that
// notation): x_j = pos_j + R_j c_j, xd_j = R_j (lin_j + ang_j x c_j),
//   com = sum m_j x_j / M,  l = sum m_j xd_j,  k = sum [R_j Ic_j ang_j + m_j (x_j - com) x xd_j],
//   T = 1/2 sum (m_j |xd_j|^2 + ang_j . Ic_j ang_j).
//
// com / centroidal: one root-to-leaf sweep over the `Topo` policy, one configuration per lane,
// link_kin_body's scheme -- the running world pose (and link velocity) of the current link plus a
// slot per branch link.  A link adds its share to the accumulators and is forgotten: with the link's
// spatial inertia at its own origin (m, h = m c, I_o: load_link) its momentum in link coordinates is
// (n, f) = I (ang, lin) (inertia_mul), which is f = m (lin + ang x c), n = Ic ang + c x f; in the
// base frame about the base origin f_b = R f, n_b = R n + pos x f_b.  So
//   m_j x_j = m pos + R h,   l += f_b,   k_O += n_b,   2 T += ang . n + lin . f
// without c_j or Ic_j (no division by a mass: massless links -- a floating base's six virtual ones --
// fold to nothing), and k = k_O - com x l once at the end.  The centre-of-mass constants rb_com
// (RB_COM_FORM) would take the same 24 FMAs per link as inertia_mul here, so these kernels are built
// without them.  Live state: pose 12 + velocity 6 + accumulators 11, whatever N for a serial chain.
//
// The sweeps run in the kernels' per-link frames whose z is the joint axis (x_urdf = R_a x_kernel, a
// rotation about the shared origin).  Every output is a base-frame quantity and the packed inertial
// constants are given in the kernel frame, so nothing has to be turned by R_a on the way out: the
// frame never reaches the caller.
//
// cmm: everything in base-frame coordinates.  The forward sweep leaves per link the joint axis
// a_j = R_j e_z, the origin p_j and the link's ten inertial numbers about the base origin
// (m_j, s_j = m_j x_j, I_j).  With hb = R h and B(p, u) = (p . u) 1 - (p u^T + u p^T) / 2
//   I_j = R I_o R^T + B(p, m p + 2 hb)
// (the parallel-axis terms of moving I_o from the link origin to the base origin, again without c).
// A leaf-to-root sweep adds each link's ten numbers into its parent -- plain sums, one frame -- which
// gives the subtree composites m^C, s^C, I^C; column k is the momentum of subtree k under the unit
// joint motion, shifted to com:
//   revolute   l = a x (s^C - m^C p),  k_O = I^C a - s^C x (a x p)
//   prismatic  l = m^C a,              k_O = s^C x a
//   k = k_O - com x l
// stored as it completes.  16 values per link are live between the sweeps.
//
// Every input goes through the InputGuard before the first row is stored and every output leaves
// through lk_out (an A_G entry or a com row can be a bare hardware sin / cos result times a folded
// constant): an out-of-domain configuration gets NaN in every element of every output.
#pragma once

#include "link_kin_body.hip.hpp"

namespace rbamd {
namespace dev {

// Root-to-leaf sweep: visit(jc, L, X, V) with link j's constants, world pose and (VEL) link velocity
// in link coordinates, as link_pose_eval / link_vel_eval carry them.  qdv is read only when VEL.
template <typename T, int N, bool FAST, typename Topo, bool VEL, typename F>
RB_HD void cz_sweep(const T *mdl, const T (&qv)[N], const T (&qdv)[N], F &&visit) {
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
        LkVel<T> V;
        V.w = v3(T(0), T(0), T(0));
        V.v = V.w;
        if constexpr (p < 0) {  // a root link: its frame in the base, the base at rest
            X.R = E;
            X.p = r;
        } else {
            LkPose<T> P;
            if constexpr (p == j - 1) P = cur; else P = kept[lk_slot<Topo, N>(p)];
            X.p = mul_add(P.p, P.R, r);
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    X.R.m[3 * a + b] = fmadd(P.R.m[3 * a + 0], E.m[b],
                                             fmadd(P.R.m[3 * a + 1], E.m[3 + b], P.R.m[3 * a + 2] * E.m[6 + b]));
            if constexpr (VEL) {
                LkVel<T> PV;
                if constexpr (p == j - 1) PV = vcur; else PV = vkept[lk_slot<Topo, N>(p)];
                V.w = mul_t(E, PV.w);
                V.v = mul_t(E, cross_sub(PV.v, r, PV.w));
            }
        }
        if constexpr (VEL) {
            if constexpr (!pri) V.w.z += qdv[j]; else V.v.z += qdv[j];  // S = (e_z, 0) / (0, e_z)
        }
        cur = X;
        vcur = V;
        if constexpr (lk_branch<Topo, N>(j)) {
            kept[lk_slot<Topo, N>(j)] = X;
            vkept[lk_slot<Topo, N>(j)] = V;
        }
        visit(jc, L, X, V);
    });
}

// s + m p + R h: link j's m_j x_j added to the running first moment.
template <typename T>
RB_HD V3<T> cz_first_moment(const V3<T> &s, const Link<T> &L, const LkPose<T> &X) {
    return mul_add(v3(fmadd(L.m, X.p.x, s.x), fmadd(L.m, X.p.y, s.y), fmadd(L.m, X.p.z, s.z)), X.R, L.h);
}

// ------------------------------------------------------------------------------- com
// out(row, value) over 3 rows.
template <typename T, int N, bool FAST, typename Topo, typename Out>
RB_HD void com_eval(const T *mdl, const T (&qv)[N], Out &&out) {
    InputGuard<T> gd;
    gd.template joints<Topo>(qv);
    V3<T> s = v3(T(0), T(0), T(0));
    T M = T(0);
    cz_sweep<T, N, FAST, Topo, false>(mdl, qv, qv, [&](auto, const Link<T> &L, const LkPose<T> &X, const LkVel<T> &) {
        M += L.m;
        s = cz_first_moment(s, L, X);
    });
    const T iM = T(1) / M;
    out(0, lk_out(gd, s.x * iM));
    out(1, lk_out(gd, s.y * iM));
    out(2, lk_out(gd, s.z * iM));
}

// ------------------------------------------------------------------------ centroidal
// out_com(row, value) over 3 rows, out_hg over 6, out_en over 2 (T, U).
template <typename T, int N, bool FAST, typename Topo, typename OutC, typename OutH, typename OutE>
RB_HD void centroidal_eval(const T *mdl, const T (&qv)[N], const T (&qdv)[N], OutC &&out_com, OutH &&out_hg,
                           OutE &&out_en) {
    InputGuard<T> gd;
    gd.template joints<Topo>(qv);
    gd.vals(qdv);
    V3<T> s = v3(T(0), T(0), T(0)), l = s, k = s;
    T M = T(0), T2 = T(0);
    cz_sweep<T, N, FAST, Topo, true>(mdl, qv, qdv, [&](auto, const Link<T> &L, const LkPose<T> &X, const LkVel<T> &V) {
        M += L.m;
        s = cz_first_moment(s, L, X);
        V3<T> n, f;
        inertia_mul(L, V.w, V.v, n, f);
        T2 = fmadd(V.w.x, n.x, fmadd(V.w.y, n.y, fmadd(V.w.z, n.z, T2)));
        T2 = fmadd(V.v.x, f.x, fmadd(V.v.y, f.y, fmadd(V.v.z, f.z, T2)));
        const V3<T> fb = mul(X.R, f);
        l = add3(l, fb);
        k = cross_add(mul_add(k, X.R, n), X.p, fb);  // about the base origin
    });
    const T iM = T(1) / M;
    const V3<T> com = v3(s.x * iM, s.y * iM, s.z * iM);
    k = cross_sub(k, com, l);  // about com
    out_com(0, lk_out(gd, com.x));
    out_com(1, lk_out(gd, com.y));
    out_com(2, lk_out(gd, com.z));
    out_hg(0, lk_out(gd, l.x));
    out_hg(1, lk_out(gd, l.y));
    out_hg(2, lk_out(gd, l.z));
    out_hg(3, lk_out(gd, k.x));
    out_hg(4, lk_out(gd, k.y));
    out_hg(5, lk_out(gd, k.z));
    out_en(0, lk_out(gd, T(0.5) * T2));
    out_en(1, lk_out(gd, T(kGravity) * M * com.z));
}

// ------------------------------------------------------------------------------- cmm
// A link's (then a subtree's) inertia about the base origin, base axes.
template <typename T>
struct CzInertia {
    T m;
    V3<T> s;
    S3<T> I;
};

template <typename T>
RB_HD CzInertia<T> cz_link_inertia(const Link<T> &L, const LkPose<T> &X) {
    const M3<T> &R = X.R;
    const V3<T> &p = X.p;
    const V3<T> hb = mul(R, L.h);
    CzInertia<T> c;
    c.m = L.m;
    c.s = v3(fmadd(L.m, p.x, hb.x), fmadd(L.m, p.y, hb.y), fmadd(L.m, p.z, hb.z));
    // G = R I_o, then R I_o R^T
    T G[9];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const V3<T> g = mul(L.Io, v3(R.m[3 * a + 0], R.m[3 * a + 1], R.m[3 * a + 2]));
        G[3 * a + 0] = g.x;
        G[3 * a + 1] = g.y;
        G[3 * a + 2] = g.z;
    }
    auto rot = [&](int a, int b, T acc) {
        return fmadd(G[3 * a + 0], R.m[3 * b + 0], fmadd(G[3 * a + 1], R.m[3 * b + 1], fmadd(G[3 * a + 2], R.m[3 * b + 2], acc)));
    };
    // B(p, u), u = m p + 2 hb = s + hb
    const V3<T> u = add3(c.s, hb);
    const T h = T(0.5);
    c.I.xx = rot(0, 0, fmadd(p.y, u.y, p.z * u.z));
    c.I.yy = rot(1, 1, fmadd(p.x, u.x, p.z * u.z));
    c.I.zz = rot(2, 2, fmadd(p.x, u.x, p.y * u.y));
    c.I.xy = rot(0, 1, -h * fmadd(p.x, u.y, u.x * p.y));
    c.I.xz = rot(0, 2, -h * fmadd(p.x, u.z, u.x * p.z));
    c.I.yz = rot(1, 2, -h * fmadd(p.y, u.z, u.y * p.z));
    return c;
}

template <typename T>
RB_HD void cz_add(CzInertia<T> &a, const CzInertia<T> &b) {
    a.m += b.m;
    a.s = add3(a.s, b.s);
    a.I = S3<T>{a.I.xx + b.I.xx, a.I.xy + b.I.xy, a.I.xz + b.I.xz, a.I.yy + b.I.yy, a.I.yz + b.I.yz, a.I.zz + b.I.zz};
}

// out(row, value) over 6 N rows, column by column from the last link to the first.
template <typename T, int N, bool FAST, typename Topo, typename Out>
RB_HD void cmm_eval(const T *mdl, const T (&qv)[N], Out &&out) {
    InputGuard<T> gd;
    gd.template joints<Topo>(qv);
    V3<T> ax[N], org[N];
    CzInertia<T> C[N];
    V3<T> s = v3(T(0), T(0), T(0));
    T M = T(0);
    cz_sweep<T, N, FAST, Topo, false>(mdl, qv, qv, [&](auto jc, const Link<T> &L, const LkPose<T> &X, const LkVel<T> &) {
        constexpr int j = decltype(jc)::value;
        ax[j] = v3(X.R.m[2], X.R.m[5], X.R.m[8]);
        org[j] = X.p;
        C[j] = cz_link_inertia(L, X);
        M += L.m;
        s = add3(s, C[j].s);
    });
    const T iM = T(1) / M;
    const V3<T> com = v3(s.x * iM, s.y * iM, s.z * iM);
    cfor_rev<N>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr int p = Topo::parent(j);
        const V3<T> a = ax[j];
        const CzInertia<T> &c = C[j];
        V3<T> l, k;
        if constexpr (!Topo::prismatic(j)) {
            const V3<T> o = org[j];
            l = cross(a, v3(fmadd(-c.m, o.x, c.s.x), fmadd(-c.m, o.y, c.s.y), fmadd(-c.m, o.z, c.s.z)));
            k = cross_sub(mul(c.I, a), c.s, cross(a, o));
        } else {
            l = v3(c.m * a.x, c.m * a.y, c.m * a.z);
            k = cross(c.s, a);
        }
        k = cross_sub(k, com, l);
        out(6 * j + 0, lk_out(gd, l.x));
        out(6 * j + 1, lk_out(gd, l.y));
        out(6 * j + 2, lk_out(gd, l.z));
        out(6 * j + 3, lk_out(gd, k.x));
        out(6 * j + 4, lk_out(gd, k.y));
        out(6 * j + 5, lk_out(gd, k.z));
        if constexpr (p >= 0) cz_add(C[p], C[j]);
    });
}

// ---------------------------------------------------------------------- lane bodies
// One configuration per lane on SoA rows; the inputs are loaded up front (every one is checked
// before the first store), the outputs stored under the RB_NT policy.
template <typename T, int N, bool FAST, typename Topo = SerialTopo>
__device__ __forceinline__ void com_lane(const T *mdl, const T *__restrict__ q, T *__restrict__ com, uint32_t b,
                                         int64_t ld) {
    const uint32_t off = b * (uint32_t)sizeof(T);
    T qv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) qv[j] = ld_row(q, j * ld, off);
    com_eval<T, N, FAST, Topo>(mdl, qv, [&](int e, T v) { st_row(com, e * ld, off, v); });
}

template <typename T, int N, bool FAST, typename Topo = SerialTopo>
__device__ __forceinline__ void centroidal_lane(const T *mdl, const T *__restrict__ q, const T *__restrict__ qd,
                                                T *__restrict__ com, T *__restrict__ hg, T *__restrict__ energy,
                                                uint32_t b, int64_t ld) {
    const uint32_t off = b * (uint32_t)sizeof(T);
    T qv[N], qdv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        qv[j] = ld_row(q, j * ld, off);
        qdv[j] = ld_row(qd, j * ld, off);
    }
    centroidal_eval<T, N, FAST, Topo>(
        mdl, qv, qdv, [&](int e, T v) { st_row(com, e * ld, off, v); }, [&](int e, T v) { st_row(hg, e * ld, off, v); },
        [&](int e, T v) { st_row(energy, e * ld, off, v); });
}

template <typename T, int N, bool FAST, typename Topo = SerialTopo>
__device__ __forceinline__ void cmm_lane(const T *mdl, const T *__restrict__ q, T *__restrict__ ag, uint32_t b,
                                         int64_t ld) {
    const uint32_t off = b * (uint32_t)sizeof(T);
    T qv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) qv[j] = ld_row(q, j * ld, off);
    cmm_eval<T, N, FAST, Topo>(mdl, qv, [&](int e, T v) { st_row(ag, e * ld, off, v); });
}

}  // namespace dev
}  // namespace rbamd
