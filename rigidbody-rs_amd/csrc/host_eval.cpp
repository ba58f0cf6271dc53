// host_eval.cpp -- the reference's single-configuration queries on the host CPU.
//
// SURVEY §8(d) config 1 is the reference's CPU path: one configuration per call
// (rigidbody_bindings/src/lib.rs:15-70, timed by main.cpp:69).  A GPU round trip (H2D copy,
// launch, D2H copy, stream sync) costs ~18 us there against ~0.7 us for the CPU recursion,
// so multibody_rnea / _crba / _fwd_kin / _jac evaluate the configuration on the calling
// thread -- with the SAME lane bodies the GPU kernels run (rnea_body / crba_body /
// tree_body .hip.hpp are host+device, RB_HD), instantiated here for the host against the
// packed fp64 model the precompiled kernels stage into LDS.  This is not a fallback: it is
// the single-configuration dispatch (capi.cpp single_dispatch); every batched entry point
// runs on the GPU only.  Serial revolute chains of a precompiled DOF (dofs.hpp) only; tree
// models keep the GPU path (their topology is compiled in by hipRTC).  Needs FMA3 + AVX2 on the host
// (the recursion is written in fused multiply-adds); without it the GPU path serves.
#include "host_eval.hpp"

#include <vector>

#include "rollout_vjp_body.hip.hpp"  // first: rnea_deriv_body declares the host reciprocal fdh_body's L D L^T takes
#include "crba_body.hip.hpp"
#include "dofs.hpp"
#include "centroidal_body.hip.hpp"
#include "contact_body.hip.hpp"
#include "contact_vjp_body.hip.hpp"
#include "ext_body.hip.hpp"
#include "kernels.hpp"
#include "link_kin_body.hip.hpp"
#include "rnea_body.hip.hpp"
#include "rnea_vjp_body.hip.hpp"
#include "fd_vjp_body.hip.hpp"

namespace rbamd {
namespace {

// The reference's serial chain as a full topology policy, so the tree forms of FK / the
// Jacobian (tree_body.hip.hpp) evaluate it: every link is on the last link's path.
template <int N>
struct HostSerialTopo {
    static constexpr bool kSerial = true;
    static constexpr int parent(int j) { return j - 1; }
    static constexpr bool prismatic(int) { return false; }
    static constexpr int last_child(int j) { return j + 1 < N ? j + 1 : -1; }
    static constexpr bool is_ancestor(int a, int i) { return a < i; }
    static constexpr int child_toward(int a, int i) { return a < i ? a + 1 : -1; }
    static constexpr bool on_path(int) { return true; }
};

#define RB_HOST_FMA __attribute__((target("avx2,fma")))

RB_HOST_FMA bool rnea_fma(int n, const double *mdl, const double *q, const double *qd, const double *qdd,
                          double *tau) {
    switch (n) {
#define X(N)                                                                                        \
    case N: {                                                                                       \
        double a[N], b[N], c[N];                                                                    \
        for (int j = 0; j < N; ++j) {                                                               \
            a[j] = q[j];                                                                            \
            b[j] = qd[j];                                                                           \
            c[j] = qdd[j];                                                                          \
        }                                                                                           \
        dev::rnea_eval<double, N, false>(mdl, a, b, c, [&](int j, double v) { tau[j] = v; });       \
        return true;                                                                                \
    }
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

RB_HOST_FMA bool crba_fma(int n, const double *mdl, const double *q, double *H) {
    switch (n) {
#define X(N)                                                                                        \
    case N: {                                                                                       \
        double a[N];                                                                                \
        for (int j = 0; j < N; ++j) a[j] = q[j];                                                    \
        dev::crba_eval<double, N, false>(mdl, a, [&](int e, double v) { H[e] = v; });               \
        return true;                                                                                \
    }
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

RB_HOST_FMA bool fwd_kin_fma(int n, const double *mdl, const double *q, double *pos) {
    switch (n) {
#define X(N)                                                                                        \
    case N: {                                                                                       \
        double a[N];                                                                                \
        for (int j = 0; j < N; ++j) a[j] = q[j];                                                    \
        dev::fwd_kin_tree<double, N, false, HostSerialTopo<N>>(mdl, a, [&](int e, double v) { pos[e] = v; }); \
        return true;                                                                                \
    }
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

RB_HOST_FMA bool jac_fma(int n, const double *mdl, const double *q, double *J) {
    switch (n) {
#define X(N)                                                                                        \
    case N: {                                                                                       \
        double a[N];                                                                                \
        for (int j = 0; j < N; ++j) a[j] = q[j];                                                    \
        dev::jac_tree<double, N, false, HostSerialTopo<N>>(mdl, a, [&](int e, double v) { J[e] = v; }); \
        return true;                                                                                \
    }
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

RB_HOST_FMA bool rnea_deriv_fma(int n, const double *mdl, const double *q, const double *qd, const double *qdd,
                                double *dq, double *dqd) {
    switch (n) {
#define X(N)                                                                                        \
    case N: {                                                                                       \
        double a[N], b[N], c[N];                                                                    \
        for (int j = 0; j < N; ++j) {                                                               \
            a[j] = q[j];                                                                            \
            b[j] = qd[j];                                                                           \
            c[j] = qdd[j];                                                                          \
        }                                                                                           \
        dev::rnea_deriv_eval<double, N, false>(                                                     \
            mdl, a, b, c, dq != nullptr, dqd != nullptr, [&](int e, double v) { dq[e] = v; },       \
            [&](int e, double v) { dqd[e] = v; });                                                  \
        return true;                                                                                \
    }
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

template <int N>
RB_HOST_FMA bool fd_deriv_fma_n(const double *mdl, const double *q, const double *qd, const double *tau, double *qdd,
                                double *dq, double *dqd, double *dtau) {
    if constexpr (N <= kHostFdDerivMaxLinks) {
        double a[N], b[N];
        for (int j = 0; j < N; ++j) {
            a[j] = q[j];
            b[j] = qd[j];
        }
        dev::fd_deriv_eval<double, N, false>(
            mdl, a, b,
            [&](double(&tv)[N]) {
                for (int j = 0; j < N; ++j) tv[j] = tau[j];
            },
            dq != nullptr, dqd != nullptr, dtau != nullptr,
            [&](int j, double v) {
                if (qdd) qdd[j] = v;
            },
            [&](int e, double v) { dq[e] = v; }, [&](int e, double v) { dqd[e] = v; },
            [&](int e, double v) { dtau[e] = v; });
        return true;
    } else {
        return false;
    }
}

RB_HOST_FMA bool fd_deriv_fma(int n, const double *mdl, const double *q, const double *qd, const double *tau,
                              double *qdd, double *dq, double *dqd, double *dtau) {
    switch (n) {
#define X(N) \
    case N: return fd_deriv_fma_n<N>(mdl, q, qd, tau, qdd, dq, dqd, dtau);
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

// The model's contact set as contact_body's `Con`: run-time values, a slot per point at most.
template <int N>
struct HostCon {
    static constexpr int kSlots = kContactMaxPoints;
    const ContactSet &c;
    int slot[N];
    explicit HostCon(const ContactSet &set) : c(set) {
        int slots = 0;
        for (int j = 0; j < N; ++j) {
            slot[j] = -1;
            for (int p = 0; p < c.n_points && slot[j] < 0; ++p)
                if (c.link[p] == j) slot[j] = slots++;
        }
    }
    int points() const { return c.n_points; }
    int link(int p) const { return c.link[p]; }
    int slot_of(int j) const { return slot[j]; }
    double point(int p, int k) const { return c.point[p][k]; }
    double normal(int k) const { return c.normal[k]; }
    double offset() const { return c.offset; }
    double stiffness() const { return c.stiffness; }
    double damping() const { return c.damping; }
    double friction() const { return c.friction; }
    double slip_velocity() const { return c.slip_velocity; }
};

// cs: the contact set of the contact rollout's gradient (contact_vjp_body.hip.hpp; ra its axis
// frames), NULL for the contact-free rollout's.
template <int N>
RB_HOST_FMA bool rollout_vjp_fma_n(const ContactSet *cs, const double *mdl, const double *ra, const double *q,
                                   const double *qd, const double *tau_seq, double dt, int K, const double *gq,
                                   const double *gqd, double *g_q0, double *g_qd0, double *g_tau, double *work) {
    if constexpr (N <= kHostFdDerivMaxLinks) {
        double a[N], b[N];
        for (int j = 0; j < N; ++j) {
            a[j] = q[j];
            b[j] = qd[j];
        }
        auto load_tau = [&](int k, double(&tv)[N]) {
            for (int j = 0; j < N; ++j) tv[j] = tau_seq[(size_t)k * N + j];
        };
        auto load_g = [&](int k, double(&x)[N], double(&y)[N]) {
            for (int j = 0; j < N; ++j) {
                x[j] = gq[(size_t)k * N + j];
                y[j] = gqd[(size_t)k * N + j];
            }
        };
        auto work_st = [&](int k, int r, double v) { work[(size_t)k * 2 * N + r] = v; };
        auto work_ld = [&](int k, int r) { return work[(size_t)k * 2 * N + r]; };
        auto out_tau = [&](int k, int j, double v) { g_tau[(size_t)k * N + j] = v; };
        auto out_state = [&](int j, double x, double y) {
            g_q0[j] = x;
            g_qd0[j] = y;
        };
        if (cs)
            dev::rollout_contact_vjp_eval<double, N, false, HostSerialTopo<N>>(
                mdl, ra, HostCon<N>(*cs), a, b, dt, K, load_tau, load_g, work_st, work_ld, out_tau, out_state);
        else
            dev::rollout_vjp_eval<double, N, false>(mdl, a, b, dt, K, load_tau, load_g, work_st, work_ld, out_tau,
                                                    out_state);
        return true;
    } else {
        return false;
    }
}

RB_HOST_FMA bool rollout_vjp_fma(int n, const ContactSet *cs, const double *mdl, const double *ra, const double *q,
                                 const double *qd, const double *tau_seq, double dt, int K, const double *gq,
                                 const double *gqd, double *g_q0, double *g_qd0, double *g_tau, double *work) {
    switch (n) {
#define X(N) \
    case N: return rollout_vjp_fma_n<N>(cs, mdl, ra, q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau, work);
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

RB_HOST_FMA bool rnea_ext_fma(int n, const double *mdl, const double *ra, const double *q, const double *qd,
                              const double *qdd, const double *fext, double *tau) {
    switch (n) {
#define X(N)                                                                                        \
    case N: {                                                                                       \
        double a[N], b[N], c[N];                                                                    \
        for (int j = 0; j < N; ++j) {                                                               \
            a[j] = q[j];                                                                            \
            b[j] = qd[j];                                                                           \
            c[j] = qdd[j];                                                                          \
        }                                                                                           \
        dev::rnea_ext_eval<double, N, false, HostSerialTopo<N>>(                                    \
            mdl, ra, a, b, c, [&](int r) { return fext[r]; }, [&](int j, double v) { tau[j] = v; }); \
        return true;                                                                                \
    }
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

// The mass-matrix form up to kHostFdDerivMaxLinks links, the ABA beyond (the fd_form policy's
// default; the tuning knob is not read here).
template <int N>
RB_HOST_FMA bool fd_ext_fma_n(const double *mdl, const double *ra, const double *q, const double *qd,
                              const double *tau, const double *fext, double *qdd) {
    double a[N], b[N], t[N];
    for (int j = 0; j < N; ++j) {
        a[j] = q[j];
        b[j] = qd[j];
        t[j] = tau[j];
    }
    auto fx = [&](int r) { return fext[r]; };
    auto out = [&](int j, double v) { qdd[j] = v; };
    if constexpr (N <= kHostFdDerivMaxLinks) {
        dev::fdh_ext_eval<double, N, false, HostSerialTopo<N>>(
            mdl, ra, a, b, fx,
            [&](double(&tv)[N]) {
                for (int j = 0; j < N; ++j) tv[j] = t[j];
            },
            out);
    } else {
        dev::aba_ext_eval<double, N, false, HostSerialTopo<N>>(mdl, ra, a, b, t, fx, out);
    }
    return true;
}

RB_HOST_FMA bool fd_ext_fma(int n, const double *mdl, const double *ra, const double *q, const double *qd,
                            const double *tau, const double *fext, double *qdd) {
    switch (n) {
#define X(N) \
    case N: return fd_ext_fma_n<N>(mdl, ra, q, qd, tau, fext, qdd);
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

RB_HOST_FMA bool link_pose_fma(int n, const double *mdl, const double *ra, const double *q, double *pos, double *rot) {
    switch (n) {
#define X(N)                                                                                        \
    case N: {                                                                                       \
        double a[N];                                                                                \
        for (int j = 0; j < N; ++j) a[j] = q[j];                                                    \
        dev::link_pose_eval<double, N, false, HostSerialTopo<N>>(                                   \
            mdl, ra, a, [&](int e, double v) { pos[e] = v; }, [&](int e, double v) { rot[e] = v; }); \
        return true;                                                                                \
    }
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

RB_HOST_FMA bool link_vel_fma(int n, const double *mdl, const double *ra, const double *q, const double *qd,
                              double *vel) {
    switch (n) {
#define X(N)                                                                                        \
    case N: {                                                                                       \
        double a[N], b[N];                                                                          \
        for (int j = 0; j < N; ++j) {                                                               \
            a[j] = q[j];                                                                            \
            b[j] = qd[j];                                                                           \
        }                                                                                           \
        dev::link_vel_eval<double, N, false, HostSerialTopo<N>>(mdl, ra, a, b,                      \
                                                                [&](int e, double v) { vel[e] = v; }); \
        return true;                                                                                \
    }
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

// which: 0 com (out0), 1 centroidal (out0 com, out1 hg, out2 energy), 2 cmm (out0)
RB_HOST_FMA bool centroidal_fma(int n, int which, const double *mdl, const double *q, const double *qd, double *out0,
                                double *out1, double *out2) {
    switch (n) {
#define X(N)                                                                                        \
    case N: {                                                                                       \
        double a[N], b[N];                                                                          \
        for (int j = 0; j < N; ++j) {                                                               \
            a[j] = q[j];                                                                            \
            b[j] = qd ? qd[j] : 0.0;                                                                \
        }                                                                                           \
        auto o0 = [&](int e, double v) { out0[e] = v; };                                            \
        if (which == 0)                                                                             \
            dev::com_eval<double, N, false, HostSerialTopo<N>>(mdl, a, o0);                         \
        else if (which == 2)                                                                        \
            dev::cmm_eval<double, N, false, HostSerialTopo<N>>(mdl, a, o0);                         \
        else                                                                                        \
            dev::centroidal_eval<double, N, false, HostSerialTopo<N>>(                              \
                mdl, a, b, o0, [&](int e, double v) { out1[e] = v; }, [&](int e, double v) { out2[e] = v; }); \
        return true;                                                                                \
    }
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

RB_HOST_FMA bool contact_wrench_fma(int n, const ContactSet &cs, const double *mdl, const double *ra, const double *q,
                                    const double *qd, double *fext, double *cforce) {
    switch (n) {
#define X(N)                                                                                        \
    case N: {                                                                                       \
        double a[N], b[N];                                                                          \
        for (int j = 0; j < N; ++j) {                                                               \
            a[j] = q[j];                                                                            \
            b[j] = qd[j];                                                                           \
        }                                                                                           \
        dev::contact_wrench_eval<double, N, false, HostSerialTopo<N>>(                              \
            mdl, ra, HostCon<N>(cs), a, b, [&](int e, double v) { fext[e] = v; },                   \
            [&](int e, double v) { cforce[e] = v; });                                               \
        return true;                                                                                \
    }
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

template <int N>
RB_HOST_FMA bool rollout_contact_fma_n(const ContactSet &cs, const double *mdl, const double *ra, double *q, double *qd,
                                       const double *tau_seq, double dt, int K, double *traj) {
    double a[N], b[N];
    for (int j = 0; j < N; ++j) {
        a[j] = q[j];
        b[j] = qd[j];
    }
    dev::rollout_contact_steps<double, N, false, HostSerialTopo<N>, (N <= kHostFdDerivMaxLinks)>(
        mdl, ra, HostCon<N>(cs), a, b, dt, K,
        [&](int k, double(&tv)[N]) {
            for (int j = 0; j < N; ++j) tv[j] = tau_seq[(size_t)k * N + j];
        },
        [&](int k, int j, double v) { traj[(size_t)k * N + j] = v; });
    for (int j = 0; j < N; ++j) {
        q[j] = a[j];
        qd[j] = b[j];
    }
    return true;
}

RB_HOST_FMA bool rollout_contact_fma(int n, const ContactSet &cs, const double *mdl, const double *ra, double *q,
                                     double *qd, const double *tau_seq, double dt, int K, double *traj) {
    switch (n) {
#define X(N) \
    case N: return rollout_contact_fma_n<N>(cs, mdl, ra, q, qd, tau_seq, dt, K, traj);
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

// fext NULL: the plain RNEA's gradient (g_fext unused); g_fext NULL: not evaluated.
template <int N>
RB_HOST_FMA bool rnea_vjp_fma_n(const double *mdl, const double *ra, const double *q, const double *qd,
                                const double *qdd, const double *fext, const double *w, double *g_q, double *g_qd,
                                double *g_qdd, double *g_fext) {
    double a[N], b[N], c[N], d[N];
    for (int j = 0; j < N; ++j) {
        a[j] = q[j];
        b[j] = qd[j];
        c[j] = qdd[j];
        d[j] = w[j];
    }
    auto fx = [&](int r) { return fext[r]; };
    auto oq = [&](int j, double v) { g_q[j] = v; };
    auto oqd = [&](int j, double v) { g_qd[j] = v; };
    auto oqdd = [&](int j, double v) { g_qdd[j] = v; };
    auto of = [&](int r, double v) { g_fext[r] = v; };
    if (fext)
        dev::rnea_vjp_eval<double, N, false, HostSerialTopo<N>, true>(mdl, ra, a, b, c, d, fx, g_fext != nullptr, oq, oqd,
                                                                      oqdd, of);
    else
        dev::rnea_vjp_eval<double, N, false, HostSerialTopo<N>, false>(mdl, ra, a, b, c, d, fx, false, oq, oqd, oqdd, of);
    return true;
}

RB_HOST_FMA bool rnea_vjp_fma(int n, const double *mdl, const double *ra, const double *q, const double *qd,
                              const double *qdd, const double *fext, const double *w, double *g_q, double *g_qd,
                              double *g_qdd, double *g_fext) {
    switch (n) {
#define X(N) \
    case N: return rnea_vjp_fma_n<N>(mdl, ra, q, qd, qdd, fext, w, g_q, g_qd, g_qdd, g_fext);
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

// fext NULL: the gradient without wrench rows (g_fext unused); g_fext NULL: not evaluated.  The forward
// stage takes fd_ext_fma_n's form: the mass-matrix form up to kHostFdDerivMaxLinks links, the ABA beyond.
template <int N>
RB_HOST_FMA bool fd_vjp_fma_n(const double *mdl, const double *ra, const double *q, const double *qd, const double *tau,
                              const double *fext, const double *w, double *qdd, double *g_q, double *g_qd,
                              double *g_tau, double *g_fext) {
    double a[N], b[N];
    for (int j = 0; j < N; ++j) {
        a[j] = q[j];
        b[j] = qd[j];
    }
    auto fx = [&](int r) { return fext[r]; };
    auto tw = [&](double(&tv)[N], double(&wv)[N]) {
        for (int j = 0; j < N; ++j) {
            tv[j] = tau[j];
            wv[j] = w[j];
        }
    };
    auto oqdd = [&](int j, double v) { qdd[j] = v; };
    auto oq = [&](int j, double v) { g_q[j] = v; };
    auto oqd = [&](int j, double v) { g_qd[j] = v; };
    auto ot = [&](int j, double v) { g_tau[j] = v; };
    auto of = [&](int r, double v) { g_fext[r] = v; };
    constexpr bool fdh = N <= kHostFdDerivMaxLinks;
    if (fext)
        dev::fd_vjp_eval<double, N, false, HostSerialTopo<N>, true, fdh>(mdl, ra, a, b, fx, tw, g_fext != nullptr, oqdd, oq,
                                                                         oqd, ot, of);
    else
        dev::fd_vjp_eval<double, N, false, HostSerialTopo<N>, false, fdh>(mdl, ra, a, b, fx, tw, false, oqdd, oq, oqd, ot,
                                                                          of);
    return true;
}

RB_HOST_FMA bool fd_vjp_fma(int n, const double *mdl, const double *ra, const double *q, const double *qd,
                            const double *tau, const double *fext, const double *w, double *qdd, double *g_q,
                            double *g_qd, double *g_tau, double *g_fext) {
    switch (n) {
#define X(N) \
    case N: return fd_vjp_fma_n<N>(mdl, ra, q, qd, tau, fext, w, qdd, g_q, g_qd, g_tau, g_fext);
        RB_FOR_EACH_DOF(X)
#undef X
        default: return false;
    }
}

}  // namespace

bool host_fma_available() {
    static const bool ok = __builtin_cpu_supports("fma") && __builtin_cpu_supports("avx2");
    return ok;
}

bool host_eval_supported(const Model &m) { return host_fma_available() && m.serial_revolute() && dof_supported(m.n); }

bool host_rnea(const Model &m, const double *pk, const double *q, const double *qd, const double *qdd, double *tau) {
    return host_eval_supported(m) && rnea_fma(m.n, pk, q, qd, qdd, tau);
}

bool host_crba(const Model &m, const double *pk, const double *q, double *H) {
    return host_eval_supported(m) && crba_fma(m.n, pk, q, H);
}

bool host_fwd_kin(const Model &m, const double *pk, const double *q, double *pos) {
    return host_eval_supported(m) && fwd_kin_fma(m.n, pk, q, pos);
}

bool host_jac(const Model &m, const double *pk, const double *q, double *J) {
    return host_eval_supported(m) && jac_fma(m.n, pk, q, J);
}

bool host_rnea_deriv(const Model &m, const double *pk, const double *q, const double *qd, const double *qdd,
                     double *dtau_dq, double *dtau_dqd) {
    return host_eval_supported(m) && rnea_deriv_fma(m.n, pk, q, qd, qdd, dtau_dq, dtau_dqd);
}

bool host_fd_deriv(const Model &m, const double *pk, const double *q, const double *qd, const double *tau, double *qdd,
                   double *dqdd_dq, double *dqdd_dqd, double *dqdd_dtau) {
    return host_eval_supported(m) && m.n <= kHostFdDerivMaxLinks &&
           fd_deriv_fma(m.n, pk, q, qd, tau, qdd, dqdd_dq, dqdd_dqd, dqdd_dtau);
}

bool host_rollout_vjp(const Model &m, const double *pk, const double *q, const double *qd, const double *tau_seq,
                      double dt, int K, const double *gq, const double *gqd, double *g_q0, double *g_qd0,
                      double *g_tau) {
    if (!host_eval_supported(m) || m.n > kHostFdDerivMaxLinks || K < 1) return false;
    std::vector<double> work((size_t)K * 2 * m.n);
    return rollout_vjp_fma(m.n, nullptr, pk, nullptr, q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau, work.data());
}

bool host_rollout_contact_vjp(const Model &m, const double *pk, const double *ra, const double *q, const double *qd,
                              const double *tau_seq, double dt, int K, const double *gq, const double *gqd,
                              double *g_q0, double *g_qd0, double *g_tau) {
    if (!host_eval_supported(m) || m.n > kHostFdDerivMaxLinks || K < 1 || m.contacts.n_points < 1) return false;
    std::vector<double> work((size_t)K * 2 * m.n);
    return rollout_vjp_fma(m.n, &m.contacts, pk, ra, q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau, work.data());
}

bool host_rnea_ext(const Model &m, const double *pk, const double *ra, const double *q, const double *qd,
                   const double *qdd, const double *fext, double *tau) {
    return host_eval_supported(m) && rnea_ext_fma(m.n, pk, ra, q, qd, qdd, fext, tau);
}

bool host_fd_ext(const Model &m, const double *pk, const double *ra, const double *q, const double *qd,
                 const double *tau, const double *fext, double *qdd) {
    return host_eval_supported(m) && fd_ext_fma(m.n, pk, ra, q, qd, tau, fext, qdd);
}

bool host_rnea_vjp(const Model &m, const double *pk, const double *ra, const double *q, const double *qd,
                   const double *qdd, const double *fext, const double *w, double *g_q, double *g_qd, double *g_qdd,
                   double *g_fext) {
    return host_eval_supported(m) && rnea_vjp_fma(m.n, pk, ra, q, qd, qdd, fext, w, g_q, g_qd, g_qdd, g_fext);
}

bool host_fd_vjp(const Model &m, const double *pk, const double *ra, const double *q, const double *qd,
                 const double *tau, const double *fext, const double *w, double *qdd, double *g_q, double *g_qd,
                 double *g_tau, double *g_fext) {
    return host_eval_supported(m) && fd_vjp_fma(m.n, pk, ra, q, qd, tau, fext, w, qdd, g_q, g_qd, g_tau, g_fext);
}

bool host_link_pose(const Model &m, const double *pk, const double *ra, const double *q, double *pos, double *rot) {
    return host_eval_supported(m) && link_pose_fma(m.n, pk, ra, q, pos, rot);
}

bool host_link_vel(const Model &m, const double *pk, const double *ra, const double *q, const double *qd,
                   double *vel) {
    return host_eval_supported(m) && link_vel_fma(m.n, pk, ra, q, qd, vel);
}

bool host_com(const Model &m, const double *pk, const double *q, double *com) {
    return host_eval_supported(m) && centroidal_fma(m.n, 0, pk, q, nullptr, com, nullptr, nullptr);
}

bool host_centroidal(const Model &m, const double *pk, const double *q, const double *qd, double *com, double *hg,
                     double *energy) {
    return host_eval_supported(m) && centroidal_fma(m.n, 1, pk, q, qd, com, hg, energy);
}

bool host_cmm(const Model &m, const double *pk, const double *q, double *ag) {
    return host_eval_supported(m) && centroidal_fma(m.n, 2, pk, q, nullptr, ag, nullptr, nullptr);
}

bool host_contact_wrench(const Model &m, const double *pk, const double *ra, const double *q, const double *qd,
                         double *fext, double *cforce) {
    return host_eval_supported(m) && m.contacts.n_points > 0 &&
           contact_wrench_fma(m.n, m.contacts, pk, ra, q, qd, fext, cforce);
}

bool host_rollout_contact(const Model &m, const double *pk, const double *ra, double *q, double *qd,
                          const double *tau_seq, double dt, int K, double *traj) {
    return host_eval_supported(m) && m.contacts.n_points > 0 &&
           rollout_contact_fma(m.n, m.contacts, pk, ra, q, qd, tau_seq, dt, K, traj);
}

}  // namespace rbamd
