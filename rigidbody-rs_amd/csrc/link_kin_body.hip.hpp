// link_kin_body.hip.hpp -- kinematics of every link (device + host).
//
//   link_pose(q)     -> pos_j, R_j   pose of link j's URDF link frame in the base frame
//   link_vel(q, qd)  -> vel_j        spatial velocity of link j, in its own URDF link frame
//
// The frame is link j's own URDF link frame -- the joint's child frame, after the joint's motion:
// the frame fext_j of ext_body.hip.hpp is given in and fwd_kin / jac report for the last link.
//   pos  [3 N]  rows 3 j + c: component c of the frame origin in the base frame
//   rot  [9 N]  rows 9 j + row + 3 col: R_j, x_base = R_j x_link (column-major, the ABI's order)
//   vel  [6 N]  rows 6 j + 0..2 the linear velocity of the frame origin, 6 j + 3..5 the angular
//               velocity, both in link j's frame ([lin; rot], the Jacobian's and fext's row order):
//               vel_j = J_j(q) qd with J_j the body Jacobian of link j.  Purely kinematic: the
//               base does not accelerate here, gravity does not enter.
//
// One root-to-leaf sweep over the `Topo` policy (tree_body.hip.hpp), one configuration per lane;
// a link's rows are handed to `out` as soon as the link completes, so the 12 N / 6 N outputs are
// never held together.  The state a child reads is its parent's world pose (pose) or link velocity
// (vel).  Links are numbered parent before child, so the parent of link j is either link j - 1 --
// the sweep's running state `cur` -- or a link with a child other than its immediate successor, a
// branch link.  Only branch links are kept beyond the next step, each in a slot of its own
// (lk_slot), read for the last time by its last child (Topo::last_child): a serial chain keeps
// nothing but `cur`, a quadruped its trunk.  There is no per-link array of poses.
//
// The sweeps run in the kernels' per-link frames whose z is the joint axis (model.cpp pack:
// x_urdf = R_a x_kernel); `ra` holds every link's R_a (9 N, row-major, the constants the
// external-wrench kernels take) and the outputs are turned on the way out: R_urdf = R_kernel R_a^T,
// vel_urdf = R_a vel_kernel per 3-vector -- exact identities, folded away, for z-axis links.
//
// Every input goes through the InputGuard before the first row is stored (rows leave link by
// link, so the check cannot trail the sweep): an out-of-domain configuration gets NaN in every
// element of every output.
#pragma once

#include "tree_body.hip.hpp"

namespace rbamd {
namespace dev {

// Highest-index child of link j (-1: a leaf); SerialTopo does not carry it.
template <typename Topo, int N>
constexpr int lk_last_child(int j) {
    if constexpr (Topo::kSerial)
        return j + 1 < N ? j + 1 : -1;
    else
        return Topo::last_child(j);
}

// A branch link: it has a child other than link j + 1, so its state outlives the next step.
template <typename Topo, int N>
constexpr bool lk_branch(int j) {
    return lk_last_child<Topo, N>(j) > j + 1;
}

// Slot of branch link j: its rank among the branch links.
template <typename Topo, int N>
constexpr int lk_slot(int j) {
    int s = 0;
    for (int k = 0; k < j; ++k)
        if (lk_branch<Topo, N>(k)) ++s;
    return s;
}

// Number of slots (at least one, so the array exists for a serial chain too; unused there).
template <typename Topo, int N>
constexpr int lk_slots() {
    const int s = lk_slot<Topo, N>(N);
    return s > 0 ? s : 1;
}

// a rotation with unit diagonal is the identity (trace 3)
template <typename T>
RB_HD bool lk_identity(const T *r) {
    return r[0] == T(1) && r[4] == T(1) && r[8] == T(1);
}

// One output through the guard.  fp32 outputs leave through InputGuard's inline-assembly add, which
// the compiler's hazard recognizer does not look into.  Here an output can BE a hardware sin / cos
// result -- a rotation entry of a link whose R_p is a signed permutation -- and gfx950 wants one wait
// state between a transcendental instruction and a VALU instruction that reads its result: without
// it some lanes store what the register held before.  So the value first passes through a no-op
// the compiler must order between the two (fp64 outputs are not read by assembly: nothing to do).
template <typename T>
RB_HD T lk_out(const InputGuard<T> &gd, T v) {
#if RB_GUARD_ASM
    if constexpr (!__is_same(T, double)) asm("s_nop 1 ; rb_settle" : "+v"(v));
#endif
    return gd.out(v);
}

// World pose of a link's kernel frame: x_base = R x_link + p.
template <typename T>
struct LkPose {
    M3<T> R;
    V3<T> p;
};

// Link velocity (rot, lin) in link coordinates.
template <typename T>
struct LkVel {
    V3<T> w, v;
};

// ------------------------------------------------------------------------------ pose
// out_pos(row, value) over 3 N rows, out_rot(row, value) over 9 N rows, link by link.
template <typename T, int N, bool FAST, typename Topo, typename OutP, typename OutR>
RB_HD void link_pose_eval(const T *mdl, const T *ra, const T (&qv)[N], OutP &&out_pos, OutR &&out_rot) {
    InputGuard<T> gd;
    gd.template joints<Topo>(qv);
    LkPose<T> cur, kept[lk_slots<Topo, N>()];
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
        if constexpr (p < 0) {  // a root link: its frame in the base
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
        }
        cur = X;
        if constexpr (lk_branch<Topo, N>(j)) kept[lk_slot<Topo, N>(j)] = X;
        out_pos(3 * j + 0, lk_out(gd, X.p.x));
        out_pos(3 * j + 1, lk_out(gd, X.p.y));
        out_pos(3 * j + 2, lk_out(gd, X.p.z));
        // R_urdf = R_kernel R_a^T, element (a, b) at row a + 3 b
        const T *A = ra + 9 * j;
        if (lk_identity(A)) {
#pragma unroll
            for (int b = 0; b < 3; ++b)
#pragma unroll
                for (int a = 0; a < 3; ++a) out_rot(9 * j + a + 3 * b, lk_out(gd, X.R.m[3 * a + b]));
        } else {
#pragma unroll
            for (int b = 0; b < 3; ++b)
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    out_rot(9 * j + a + 3 * b,
                            lk_out(gd, fmadd(X.R.m[3 * a + 0], A[3 * b + 0],
                                         fmadd(X.R.m[3 * a + 1], A[3 * b + 1], X.R.m[3 * a + 2] * A[3 * b + 2]))));
        }
    });
}

// -------------------------------------------------------------------------- velocity
// v_j = X_j v_parent + S_j qd_j (Featherstone 2008, Table 5.1), the RNEA's velocity sweep with a
// base at rest.  out(row, value) over 6 N rows, link by link.
template <typename T, int N, bool FAST, typename Topo, typename Out>
RB_HD void link_vel_eval(const T *mdl, const T *ra, const T (&qv)[N], const T (&qdv)[N], Out &&out) {
    InputGuard<T> gd;
    gd.template joints<Topo>(qv);
    gd.vals(qdv);
    LkVel<T> cur, kept[lk_slots<Topo, N>()];
    cfor<0, N>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        constexpr int p = Topo::parent(j);
        constexpr bool pri = Topo::prismatic(j);
        LkVel<T> X;
        if constexpr (p < 0) {  // the base is at rest
            X.w = v3(T(0), T(0), T(0));
            X.v = X.w;
        } else {
            const Link<T> L = load_link(mdl, j);
            T c = T(1), s = T(0);
            if constexpr (!pri) sin_cos<FAST>(qv[j], s, c);
            M3<T> E;
            V3<T> r;
            link_frame<T, pri>(L, qv[j], c, s, E, r);
            LkVel<T> P;
            if constexpr (p == j - 1) P = cur; else P = kept[lk_slot<Topo, N>(p)];
            X.w = mul_t(E, P.w);
            X.v = mul_t(E, cross_sub(P.v, r, P.w));
        }
        if constexpr (!pri) X.w.z += qdv[j]; else X.v.z += qdv[j];  // S = (e_z, 0) / (0, e_z)
        cur = X;
        if constexpr (lk_branch<Topo, N>(j)) kept[lk_slot<Topo, N>(j)] = X;
        // vel_urdf = R_a vel_kernel
        const T *A = ra + 9 * j;
        V3<T> lin = X.v, ang = X.w;
        if (!lk_identity(A)) {
            const M3<T> Ra{{A[0], A[1], A[2], A[3], A[4], A[5], A[6], A[7], A[8]}};
            lin = mul(Ra, X.v);
            ang = mul(Ra, X.w);
        }
        out(6 * j + 0, lk_out(gd, lin.x));
        out(6 * j + 1, lk_out(gd, lin.y));
        out(6 * j + 2, lk_out(gd, lin.z));
        out(6 * j + 3, lk_out(gd, ang.x));
        out(6 * j + 4, lk_out(gd, ang.y));
        out(6 * j + 5, lk_out(gd, ang.z));
    });
}

// ---------------------------------------------------------------------- lane bodies
// One configuration per lane on SoA rows; the inputs are loaded up front (every one is checked
// before the first store), the outputs stored link by link under the RB_NT policy.
template <typename T, int N, bool FAST, typename Topo = SerialTopo>
__device__ __forceinline__ void link_pose_lane(const T *mdl, const T *ra, const T *__restrict__ q,
                                               T *__restrict__ pos, T *__restrict__ rot, uint32_t b, int64_t ld) {
    const uint32_t off = b * (uint32_t)sizeof(T);
    T qv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) qv[j] = ld_row(q, j * ld, off);
    link_pose_eval<T, N, FAST, Topo>(
        mdl, ra, qv, [&](int e, T v) { st_row(pos, e * ld, off, v); }, [&](int e, T v) { st_row(rot, e * ld, off, v); });
}

template <typename T, int N, bool FAST, typename Topo = SerialTopo>
__device__ __forceinline__ void link_vel_lane(const T *mdl, const T *ra, const T *__restrict__ q,
                                              const T *__restrict__ qd, T *__restrict__ vel, uint32_t b, int64_t ld) {
    const uint32_t off = b * (uint32_t)sizeof(T);
    T qv[N], qdv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        qv[j] = ld_row(q, j * ld, off);
        qdv[j] = ld_row(qd, j * ld, off);
    }
    link_vel_eval<T, N, FAST, Topo>(mdl, ra, qv, qdv, [&](int e, T v) { st_row(vel, e * ld, off, v); });
}

}  // namespace dev
}  // namespace rbamd
