// host_eval.hpp -- single-configuration queries on the host (see host_eval.cpp).
#pragma once

#include "model.hpp"

namespace rbamd {

// FMA3 present on this CPU (checked once).
bool host_fma_available();
// Serial revolute chain of a precompiled DOF on an FMA3 host.
bool host_eval_supported(const Model &m);

// `pk` = Model::pack_f64() (the generic kernels' constant block).  Each returns false
// (nothing written) when the model / CPU is not supported; outputs follow the reference ABI
// (lib.rs:15-70): tau[n]; H[n*n] column-major upper triangle, exact-zero lower; pos[3];
// J[6n] column-major, rows [lin; rot].
bool host_rnea(const Model &m, const double *pk, const double *q, const double *qd, const double *qdd, double *tau);
bool host_crba(const Model &m, const double *pk, const double *q, double *H);
bool host_fwd_kin(const Model &m, const double *pk, const double *q, double *pos);
bool host_jac(const Model &m, const double *pk, const double *q, double *J);

// Analytical derivatives (rnea_deriv_body.hip.hpp), n x n column-major, element i + n k =
// d out_i / d in_k; a NULL output is not evaluated.  host_fd_deriv additionally needs the
// mass-matrix forward dynamics (chains up to 12 links); it ignores the fd_form tuning.
bool host_rnea_deriv(const Model &m, const double *pk, const double *q, const double *qd, const double *qdd,
                     double *dtau_dq, double *dtau_dqd);
bool host_fd_deriv(const Model &m, const double *pk, const double *q, const double *qd, const double *tau, double *qdd,
                   double *dqdd_dq, double *dqdd_dqd, double *dqdd_dtau);
constexpr int kHostFdDerivMaxLinks = 12;

// Reverse-mode gradient of the K-step rollout (rollout_vjp_body.hip.hpp), host_fd_deriv's scope:
// tau_seq, gq, gqd, g_tau [K][n], the rest [n]; the workspace is internal.  K >= 1.
bool host_rollout_vjp(const Model &m, const double *pk, const double *q, const double *qd, const double *tau_seq,
                      double dt, int K, const double *gq, const double *gqd, double *g_q0, double *g_qd0,
                      double *g_tau);

// Dynamics under external link wrenches (ext_body.hip.hpp): fext [6 n] (link j's force, then its
// moment, in its URDF link frame), ra = Model::axis_frames().  host_fd_ext: the mass-matrix form up
// to kHostFdDerivMaxLinks links, the ABA beyond.
bool host_rnea_ext(const Model &m, const double *pk, const double *ra, const double *q, const double *qd,
                   const double *qdd, const double *fext, double *tau);
bool host_fd_ext(const Model &m, const double *pk, const double *ra, const double *q, const double *qd,
                 const double *tau, const double *fext, double *qdd);

// Reverse-mode gradient of host_rnea_ext (rnea_vjp_body.hip.hpp) for the cotangent w [n] of tau: g_q, g_qd,
// g_qdd [n], g_fext [6 n] (NULL: not evaluated).  fext NULL: the plain RNEA's gradient, g_fext unused.
bool host_rnea_vjp(const Model &m, const double *pk, const double *ra, const double *q, const double *qd,
                   const double *qdd, const double *fext, const double *w, double *g_q, double *g_qd, double *g_qdd,
                   double *g_fext);

// Reverse-mode gradient of host_fd_ext (fd_vjp_body.hip.hpp) for the cotangent w [n] of qdd: qdd (host_fd_ext's
// own, from the shared factorisation), g_q, g_qd, g_tau [n], g_fext [6 n] (NULL: not evaluated).  fext NULL:
// the gradient of the forward dynamics without wrenches, g_fext unused.
bool host_fd_vjp(const Model &m, const double *pk, const double *ra, const double *q, const double *qd,
                 const double *tau, const double *fext, const double *w, double *qdd, double *g_q, double *g_qd,
                 double *g_tau, double *g_fext);

// Kinematics of every link in its URDF link frame (link_kin_body.hip.hpp): pos [3 n] and rot [9 n]
// (link j's R_j column-major, x_base = R_j x_link), vel [6 n] (link j's linear, then angular
// velocity, in its own frame); ra = Model::axis_frames().
bool host_link_pose(const Model &m, const double *pk, const double *ra, const double *q, double *pos, double *rot);
bool host_link_vel(const Model &m, const double *pk, const double *ra, const double *q, const double *qd,
                   double *vel);

// Whole-body quantities (centroidal_body.hip.hpp): com [3]; hg [6] ([lin; ang] about com) and energy
// [2] (T, U); ag [6 n], the centroidal momentum matrix, element row + 6 col.
bool host_com(const Model &m, const double *pk, const double *q, double *com);
bool host_centroidal(const Model &m, const double *pk, const double *q, const double *qd, double *com, double *hg,
                     double *energy);
bool host_cmm(const Model &m, const double *pk, const double *q, double *ag);

// Compliant ground contact (contact_body.hip.hpp) of a model that carries a contact set: fext [6 n]
// and cforce [3 P] of one configuration; K steps of the fused rollout (q, qd overwritten with the
// final state, traj [K n]) on the forward-dynamics form host_fd_ext takes.
bool host_contact_wrench(const Model &m, const double *pk, const double *ra, const double *q, const double *qd,
                         double *fext, double *cforce);
bool host_rollout_contact(const Model &m, const double *pk, const double *ra, double *q, double *qd,
                          const double *tau_seq, double dt, int K, double *traj);

// Reverse-mode gradient of the K-step contact rollout (contact_vjp_body.hip.hpp): host_rollout_vjp's
// scope and arrays, on a model that carries a contact set.
bool host_rollout_contact_vjp(const Model &m, const double *pk, const double *ra, const double *q, const double *qd,
                              const double *tau_seq, double dt, int K, const double *gq, const double *gqd,
                              double *g_q0, double *g_qd0, double *g_tau);

}  // namespace rbamd
