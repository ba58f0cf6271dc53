/*
 * rigidbody_batch.h -- batched GPU extension of the rigidbody_bindings C ABI.
 *
 * The reference exposes one configuration per call (rigidbody_bindings/src/lib.rs:15-70).
 * These entry points evaluate B configurations per call on one MI355X (gfx950) with
 * hand-written HIP kernels.  They replace, for a batch, a loop of the reference calls:
 *
 *   multibody_rnea_batch_*     <- multibody_rnea      (lib.rs:15-30, multibody.rs:111-153)
 *   multibody_fd_batch_*       <- no reference entry point: forward dynamics defined as
 *                                 qdd = sym(H)^-1 (tau - rnea(q,qd,0)) with H from
 *                                 multibody_crba (multibody.rs:155-174) (SURVEY.md §8(a)
 *                                 A10), computed by exactly that definition fused per
 *                                 configuration (RNEA bias + CRBA + L D L^T) for serial chains
 *                                 up to 12 links, by the Articulated-Body Algorithm otherwise
 *                                 (rb_set_tuning "fd_form")
 *   multibody_rnea_fd_batch_*  <- both of the above on one (q, qd): tau = rnea(q, qd, qdd) and
 *                                 qdd' = fd(q, qd, tau_in) in one launch (SURVEY.md §8(d)
 *                                 config 4's RNEA + forward-dynamics pair)
 *   multibody_rollout_batch_*  <- K fused forward-dynamics + semi-implicit Euler steps
 *                                 (MPC shooting)
 *   multibody_crba_batch_*     <- multibody_crba      (lib.rs:32-43)
 *   multibody_fwd_kin_batch_*  <- multibody_fwd_kin   (lib.rs:46-57)
 *   multibody_jac_batch_*      <- multibody_jac       (lib.rs:60-70)
 *   multibody_rnea_deriv_batch_* / multibody_fd_deriv_batch_*
 *                              <- no reference entry point: the analytical derivatives of the
 *                                 two dynamics above with respect to q, qd (and tau), for
 *                                 trajectory optimisation ("Analytical derivatives" below)
 *
 * Layout: structure of arrays.  Joint j of configuration b lives at x[j * ld + b]
 * (ld >= batch, the leading dimension).  Matrix outputs store element e of each
 * configuration at out[e * ld + b], with e following the single-call ABI's
 * column-major order (crba: e = row + n*col; jac: e = row + 6*col; fwd_kin: e = 0..2).
 *
 * Batch size: any batch >= 0 (0 = nothing to do); one kernel launch covers at most 2^28
 * configurations (lane byte offsets are 32-bit), larger batches are split into consecutive
 * launches on the same stream (tests/test_gpu_limits.py: 2^28 + 257).  rb_fill_uniform_*
 * alone takes at most 2^28 columns per call.
 *
 * Pointers: the plain entry points take DEVICE pointers (hipMalloc'd memory on the
 * current HIP device) and enqueue asynchronously on `stream` (a hipStream_t; NULL =
 * the null stream).  The *_host variants take host pointers and block until done.
 *
 * Return value: RB_OK (0) or an rb_status error code; rb_last_error() gives a
 * thread-local message.  No entry point aborts the process.
 *
 * Reentrancy: a Multibody is immutable after construction; calls on one handle
 * from several threads are safe (device model constants are uploaded once per
 * device under a lock; the single-config ABI uses thread-local staging).
 *
 * Input domain.  The reference evaluates any f64 joint angle exactly (libm sin/cos in
 * UnitQuaternion::from_scaled_axis, joint.rs:48-50) and lets NaN / Inf flow through its
 * arithmetic.  The batched kernels are exact (at the |q| <= pi tolerances of the tests) for
 *   every input finite (|x| < 2^1017 in fp64) and every revolute angle |q_j| < 2^41 rad
 *   (fp64) / 2^22 rad (fp32)
 * -- each sincos reduces the angle exactly over that range (spatial.hip.hpp; tested in every
 * kernel form at |q| from 10 rad to just below the bound -- fp64 1e9, 1e12, 2^40, 2^41 - 4 --
 * and at exactly the bound, tests/test_gpu_domain.py).  A configuration outside it -- a NaN or
 * +-Inf in any of its inputs, or an angle past the bound -- gets NaN in EVERY output (CRBA:
 * every upper-triangle entry; the strictly-lower entries stay the ABI's exact zeros), in
 * every kernel form; the other configurations of the batch, including the other half of a
 * paired lane, are unaffected.  Rollouts check the state and tau_k every step: a trajectory
 * is NaN from the step its input went bad.  (The reference yields NaN exactly in the outputs
 * that depend on the bad input -- every torque of rnea; H and J keep the entries that do
 * not; these kernels poison the whole configuration.)  The single-configuration ABI
 * (rigidbody.h) computes every finite angle exactly, as the reference, and returns NaN
 * outputs for NaN / Inf inputs.
 *
 * Accuracy (tests/test_gpu_parity.py, test_gpu_domain.py, against the fp64 oracle).  fp64 RNEA,
 * CRBA, fwd_kin, jac: |d| <= 1e-9 (1 + |ref|) element-wise.  fp64 forward dynamics is a
 * backward-stable solve (L D L^T, or the ABA): with H_s = sym(H), C = rnea(q, qd, 0),
 *   |H_s qdd - (tau - C)|_inf <= n eps64 (|H_s|_inf |qdd|_inf + |tau - C|_inf)
 *   |qdd - qdd_exact|_inf     <= 4 eps64 cond(H_s) (1 + |qdd_exact|_inf)
 * -- at any conditioning (tested to cond(H) ~ 1e14, a floating base within 1e-6 rad of its pitch
 * singularity); for cond(H) <= ~1e4 (FR3 over its limits) that is a torque residual
 * |rnea(q, qd, qdd) - tau| <= 1e-8 (1 + |tau|).  fp32: RNEA 1e-4 (1 + |tau|) (chains past ~20
 * links column-norm-wise: root torques lose digits to cancellation in any fp32 evaluation),
 * forward dynamics |rnea64(q, qd, qdd32) - tau| <= 24 eps32 (1 + |tau| + |H_s| |qdd32|).
 */
#ifndef RIGIDBODY_BATCH_H
#define RIGIDBODY_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "rigidbody.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    RB_OK = 0,
    RB_ERR_NULL = 1,        /* NULL handle or pointer */
    RB_ERR_ARG = 2,         /* bad size / leading dimension / buffer length */
    RB_ERR_HIP = 3,         /* HIP runtime error (message in rb_last_error) */
    RB_ERR_URDF = 4,        /* URDF could not be read or parsed */
    RB_ERR_DOF = 5,         /* DOF outside the compiled kernel set */
    RB_ERR_UNSUPPORTED = 6, /* model feature outside the reference's semantics */
    RB_ERR_NUMERIC = 7      /* singular articulated inertia in FD */
} rb_status;

/* ---- model construction ------------------------------------------------------- */
/* Multibody::from_urdf (multibody.rs:65-77) on a file / an in-memory string.  Any
 * number of revolute joints for which a kernel is compiled (multibody_supported_dofs);
 * with RB_MODEL_URDF_TREE, trees / prismatic joints of up to 64 DOF (hipRTC kernels). */
Multibody *multibody_new_from_urdf(const char *path);
Multibody *multibody_new_from_urdf_string(const char *xml, size_t len);

/* Model-reading flags, beyond the reference.  0 = the reference's
 * reading: top-level joints/links paired by index, fixed joints dropped, z axes only
 * (multibody.rs:65-77, 130-138).
 *   RB_MODEL_GENERAL_AXES: any revolute axis, motion subspace S = (axis, 0).  Identical
 *     results for z-axis chains.  fwd_kin/jac stay in the URDF link frames.
 *   RB_MODEL_URDF_TREE: follow joint parent/child names from the root link; fixed joints
 *     are merged (child inertia into the parent body, origin into the next joint); the
 *     inertial-origin rpy is honoured; kinematic trees (links numbered depth-first, parent
 *     index < child index, multibody_topology) with revolute / continuous / prismatic
 *     joints; mimic joints are rejected (RB_ERR_URDF).  Trees and prismatic joints run only
 *     on model-specialised (hipRTC) kernels; fwd_kin / jac then follow the last link's
 *     ancestor path (other Jacobian columns zero), CRBA keeps the upper-triangle layout
 *     with exact zeros for unrelated joint pairs.
 *   RB_MODEL_FLOATING_BASE: a free-floating root body: six massless virtual joints first --
 *     prismatic along world x, y, z, then revolute about z, y, x (yaw / pitch / roll; the
 *     root orientation is Rz Ry Rx, singular at pitch = +-pi/2).  Implies the two flags
 *     above.  Gravity stays the reference's +9.81 base acceleration (multibody.rs:117-120),
 *     so a free fall reads qdd = (0, 0, -9.81, 0, ...). */
enum { RB_MODEL_GENERAL_AXES = 1, RB_MODEL_URDF_TREE = 2, RB_MODEL_FLOATING_BASE = 4 };
Multibody *multibody_new_from_urdf_ex(const char *path, unsigned flags);
Multibody *multibody_new_from_urdf_string_ex(const char *xml, size_t len, unsigned flags);
unsigned multibody_flags(const Multibody *mb);
/* Packed fp64 model (bit-exact), for broadcasting one model to every rank (RCCL). */
int64_t multibody_blob_size(const Multibody *mb);                 /* in doubles */
int multibody_export_blob(const Multibody *mb, double *out, int64_t len);
Multibody *multibody_new_from_blob(const double *blob, int64_t len);

int multibody_dof(const Multibody *mb);
/* Total moving mass (sum of link masses). */
double multibody_total_mass(const Multibody *mb);
/* Joint limits parsed from the URDF (NaN where absent); arrays of multibody_dof. */
int multibody_limits(const Multibody *mb, double *lower, double *upper,
                     double *velocity, double *effort);
/* Writes up to `cap` DOF values the kernels are compiled for; returns their count. */
int multibody_supported_dofs(int *out, int cap);
/* Per link: parent link index (-1 = base; the reference's chain has i - 1) and joint type
 * (0 revolute, 1 prismatic).  Either array may be NULL. */
int multibody_topology(const Multibody *mb, int *parent, int *joint_type);

/* Uploads the model constants to the current HIP device now (otherwise done lazily on
 * the first batched call); call before capturing batched calls into a hipGraph. */
int multibody_upload(const Multibody *mb);

/* Which kernel a launch of `batch` configurations (tiled != 0: the *_tiled entry points)
 * runs for this model on the current device; kind 0 = rnea, 1 = fd, 2 = crba, 3 = rollout,
 * 4 = fwd_kin, 5 = jac, 6 = rnea_fd (multibody_rnea_fd_batch_*), 7 = rnea_deriv, 8 = fd_deriv
 * (multibody_rnea_deriv_batch_* / multibody_fd_deriv_batch_*; for a model outside their scope
 * these queries return -RB_ERR_UNSUPPORTED and multibody_jit_source_ex the empty source; they
 * have no generic kernel, 0 means their calls fail).  1 = model-specialised kernel
 * compiled at first use by hipRTC (this call compiles exactly the form such a launch takes), 0 =
 * precompiled generic kernel (also when hipRTC failed; rb_last_error() holds the log -- a tree
 * model's calls then fail with RB_ERR_UNSUPPORTED; kind 6: the model has no fused kernel and
 * runs the rnea then the fd kernel).  multibody_kernel_path = a 2^20-configuration SoA launch. */
int multibody_kernel_path_ex(const Multibody *mb, int kind, int f64, int64_t batch, int tiled);
int multibody_kernel_path(const Multibody *mb, int kind, int f64);
int multibody_rnea_kernel_path(const Multibody *mb, int f64);
/* The launch form of that kernel (same resolution, compiles it if needed): 0 = precompiled
 * generic kernel, else the model-specialised kernel's configurations-per-lane form -- 1 one per
 * lane, 2 two per lane on packed fp32, 3 two per lane one after the other (the fp64 RNEA from
 * 2^19 configurations, and the fp32 RNEA of chains up to 8 links on the tiled layout from 2^19,
 * compiled there with ordinary instead of non-temporal loads / stores), 4 / 5 the bias /
 * mass-matrix wave split packed / one per lane (fp32 mass-matrix forward dynamics and rollouts
 * up to 2^17 configurations).  Negative = -status on a bad argument. */
int multibody_kernel_form_ex(const Multibody *mb, int kind, int f64, int64_t batch, int tiled);
/* Where the reference's single-configuration queries (rigidbody.h: rnea, crba, fwd_kin,
 * jac) run for this model: 0 = on the calling host thread (the GPU lane bodies compiled for
 * the host; serial revolute chains of a precompiled DOF on an FMA3/AVX2 CPU), 1 = one GPU
 * launch per call (trees / prismatic joints, or rb_set_tuning("single_gpu", 1)). */
int multibody_single_config_path(const Multibody *mb);
/* The generated source of the model-specialised kernel a launch of `batch` configurations
 * (tiled != 0: the *_tiled entry points) runs -- the same form, tail and load / store policy
 * multibody_kernel_form_ex reports, and the occupancy target the occupancy-cliff rebuild adds
 * (the source is hipRTC-compiled for gfx950 to decide it, no device needed); returns its length;
 * copies at most cap-1 bytes + NUL into buf when buf != NULL.  multibody_jit_source = a
 * 2^20-configuration SoA launch. */
int multibody_jit_source_ex(const Multibody *mb, int kind, int f64, int64_t batch, int tiled, char *buf,
                            int64_t cap);
int multibody_jit_source(const Multibody *mb, int kind, int f64, char *buf, int64_t cap);
/* hipRTC-compiles that kernel for `arch` (NULL = "gfx950") without a device; returns
 * the code-object size, or minus an rb_status code (log in rb_last_error()). */
int64_t multibody_jit_compile_ex(const Multibody *mb, int kind, int f64, int64_t batch, int tiled,
                                 const char *arch);
int64_t multibody_jit_compile(const Multibody *mb, int kind, int f64, const char *arch);

void multibody_result_free(double *p);
const char *rb_last_error(void);
const char *rb_version(void);
/* Launch-shape knobs for A/B measurements (keys and defaults: INTEGRATION.md "Knobs",
 * rigidbody-rs_amd/csrc/tuning.hpp); defaults are the tuned values.  Process-wide. */
int rb_set_tuning(const char *key, int value);

/* ---- batched device-pointer entry points (asynchronous on `stream`) ------------ */
int multibody_rnea_batch_f32(const Multibody *mb, const float *q, const float *qd,
                             const float *qdd, float *tau, int64_t batch, int64_t ld,
                             void *stream);
int multibody_rnea_batch_f64(const Multibody *mb, const double *q, const double *qd,
                             const double *qdd, double *tau, int64_t batch, int64_t ld,
                             void *stream);
int multibody_fd_batch_f32(const Multibody *mb, const float *q, const float *qd,
                           const float *tau, float *qdd, int64_t batch, int64_t ld,
                           void *stream);
int multibody_fd_batch_f64(const Multibody *mb, const double *q, const double *qd,
                           const double *tau, double *qdd, int64_t batch, int64_t ld,
                           void *stream);
/* Tiled layout (same computation): every array is [ceil(batch/256)][rows][256], element
 * (row j, configuration b) at ((b / 256) * rows + j) * 256 + b % 256, rows = n -- each
 * 256-configuration tile of all joints contiguous.  Measured on MI355X (bench.py layout_ab_*
 * lines, interleaved in one process, driver runs): fp64 RNEA 3-6% faster than SoA rows, fp32
 * RNEA ~5% faster, fp64 FD equal -- use it when the data is produced tiled, not by converting.  Allocate
 * whole tiles; lanes past `batch` in the last tile are neither read nor written. */
int multibody_rnea_batch_tiled_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                   float *tau, int64_t batch, void *stream);
int multibody_rnea_batch_tiled_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                   double *tau, int64_t batch, void *stream);
int multibody_fd_batch_tiled_f32(const Multibody *mb, const float *q, const float *qd, const float *tau,
                                 float *qdd, int64_t batch, void *stream);
int multibody_fd_batch_tiled_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                                 double *qdd, int64_t batch, void *stream);
/* Inverse and forward dynamics of the same (q, qd) in one launch:
 *   tau     = rnea(q, qd, qdd)                   (multibody_rnea_batch_*, multibody.rs:111-153)
 *   qdd_out = sym(H)^-1 (tau_in - rnea(q, qd, 0)) (multibody_fd_batch_*)
 * For models on the mass-matrix forward dynamics (serial revolute chains up to 12 links) one
 * fused kernel evaluates both from one set of factors: the bias torques C = rnea(q, qd, 0), H
 * (multibody.rs:155-174) and its L D L^T, with tau = C + sym(H) qdd -- the RNEA is affine in qdd
 * with slope H -- so q and qd are read once: 6 n s bytes per configuration against 8 n s for
 * the two calls, and one launch.  tau agrees with multibody_rnea_batch_* to rounding (not bit
 * for bit: a different order of the same sums; tested against the oracle at 1e-9 scaled in
 * fp64), qdd_out with multibody_fd_batch_* bit for bit.  Other models run the two kernels
 * back to back on `stream`.  Input domain as above, per output: tau is NaN for a configuration
 * whose q, qd or qdd is out of the domain, qdd_out for one whose q, qd or tau_in is.  Outputs
 * must not overlap the inputs or each other (an output passed as an input, e.g. tau_in as tau,
 * is refused with RB_ERR_ARG). */
int multibody_rnea_fd_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                const float *tau_in, float *tau, float *qdd_out, int64_t batch, int64_t ld,
                                void *stream);
int multibody_rnea_fd_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                const double *tau_in, double *tau, double *qdd_out, int64_t batch, int64_t ld,
                                void *stream);
int multibody_rnea_fd_batch_tiled_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                      const float *tau_in, float *tau, float *qdd_out, int64_t batch, void *stream);
int multibody_rnea_fd_batch_tiled_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                      const double *tau_in, double *tau, double *qdd_out, int64_t batch,
                                      void *stream);
/* Blocking host-pointer form ([n][batch] host arrays in and out), as the *_batch_host_* below. */
int multibody_rnea_fd_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                     const double *tau_in, double *tau, double *qdd_out, int64_t batch);
int multibody_rnea_fd_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                     const float *tau_in, float *tau, float *qdd_out, int64_t batch);
/* SoA [rows][ld] <-> tiled [ceil(batch/256)][rows][256] (to_tiled zero-fills the tail lanes). */
int rb_to_tiled_f32(const float *src, int64_t ld, float *dst, int rows, int64_t batch, void *stream);
int rb_to_tiled_f64(const double *src, int64_t ld, double *dst, int rows, int64_t batch, void *stream);
int rb_from_tiled_f32(const float *src, float *dst, int64_t ld, int rows, int64_t batch, void *stream);
int rb_from_tiled_f64(const double *src, double *dst, int64_t ld, int rows, int64_t batch, void *stream);

/* Fused rollout for MPC shooting: K steps of semi-implicit Euler on the forward dynamics
 * above (the same algorithm the fd entry points use), qd += dt * qdd(q, qd, tau_k); q += dt * qd, the state
 * kept on chip between steps (LDS for fp32 chains up to 16 links, registers otherwise; below
 * 2^17 fp32 configurations each step is split over a pair of waves sharing the state in LDS).  q and qd
 * ([n][ld]) are read and overwritten with the final state; tau_seq is [K][n][ld] (step k,
 * joint j, config b at (k*n + j)*ld + b); traj (same shape, may be NULL) receives q after
 * every step. */
int multibody_rollout_batch_f32(const Multibody *mb, float *q, float *qd, const float *tau_seq,
                                double dt, int K, float *traj, int64_t batch, int64_t ld,
                                void *stream);
int multibody_rollout_batch_f64(const Multibody *mb, double *q, double *qd, const double *tau_seq,
                                double dt, int K, double *traj, int64_t batch, int64_t ld,
                                void *stream);
int multibody_crba_batch_f32(const Multibody *mb, const float *q, float *H,
                             int64_t batch, int64_t ld, void *stream);
int multibody_crba_batch_f64(const Multibody *mb, const double *q, double *H,
                             int64_t batch, int64_t ld, void *stream);
int multibody_fwd_kin_batch_f64(const Multibody *mb, const double *q, double *pos,
                                int64_t batch, int64_t ld, void *stream);
int multibody_jac_batch_f64(const Multibody *mb, const double *q, double *J,
                            int64_t batch, int64_t ld, void *stream);
/* The same in fp32 (the reference computes them in fp64, lib.rs:46-70; fp32 for callers that
 * keep their batch in fp32). */
int multibody_fwd_kin_batch_f32(const Multibody *mb, const float *q, float *pos,
                                int64_t batch, int64_t ld, void *stream);
int multibody_jac_batch_f32(const Multibody *mb, const float *q, float *J,
                            int64_t batch, int64_t ld, void *stream);
/* The q-only queries on the tiled layout: q is [ceil(batch/256)][n][256], the output
 * [ceil(batch/256)][rows][256] with rows = n*n (crba), 6n (jac), 3 (fwd_kin), elements in the
 * same order as the SoA rows above.  Bit-identical to the SoA forms. */
int multibody_crba_batch_tiled_f32(const Multibody *mb, const float *q, float *H, int64_t batch, void *stream);
int multibody_crba_batch_tiled_f64(const Multibody *mb, const double *q, double *H, int64_t batch, void *stream);
int multibody_fwd_kin_batch_tiled_f32(const Multibody *mb, const float *q, float *pos, int64_t batch,
                                      void *stream);
int multibody_fwd_kin_batch_tiled_f64(const Multibody *mb, const double *q, double *pos, int64_t batch,
                                      void *stream);
int multibody_jac_batch_tiled_f32(const Multibody *mb, const float *q, float *J, int64_t batch, void *stream);
int multibody_jac_batch_tiled_f64(const Multibody *mb, const double *q, double *J, int64_t batch, void *stream);

/* ---- analytical derivatives of the inverse and forward dynamics ----------------- */
/* For a configuration (q, qd, qdd) of an n-DOF model, tau = rnea(q, qd, qdd):
 *   dtau_dq [i, k] = d tau_i / d q_k        dtau_dqd[i, k] = d tau_i / d qd_k
 * (d tau / d qdd is sym(H): multibody_crba_batch_*).  For (q, qd, tau), qdd = fd(q, qd, tau) as
 * multibody_fd_batch_* defines it:
 *   dqdd_dq   = -sym(H)^-1 dtau_dq (q, qd, qdd)
 *   dqdd_dqd  = -sym(H)^-1 dtau_dqd(q, qd, qdd)
 *   dqdd_dtau =  sym(H)^-1                       (full symmetric, both triangles written)
 * Layout: the matrix convention above, element e = i + n k (row i the output index, column k the
 * differentiated joint, column-major) of configuration b at out[e * ld + b]; each matrix is
 * [n * n][ld].  Any output may be NULL and is then neither computed nor stored; every output
 * NULL is RB_ERR_NULL.  qdd_out equals multibody_fd_batch_* bit for bit (the same lane
 * arithmetic).  An output that is also an input, or passed twice, is refused (RB_ERR_ARG).
 * batch >= 0, split at 2^28 per launch; ld >= batch.
 *
 * Scope: serial revolute chains (z-axis or RB_MODEL_GENERAL_AXES) of any supported length for
 * rnea_deriv (chains past 16 links run rolled loops over per-lane arrays: correct, not tuned);
 * fd_deriv on the mass-matrix forward dynamics only (chains up to 12 links).  Kinematic trees,
 * prismatic joints, a floating base, and fd_deriv on longer chains return RB_ERR_UNSUPPORTED;
 * rb_last_error() names the condition.  The batched forms run on model-specialised (hipRTC)
 * kernels only (kinds 7 and 8): with hipRTC disabled or failed they return RB_ERR_UNSUPPORTED
 * with the log.  SoA rows only (no tiled form).
 *
 * Algorithm (rnea_deriv_body.hip.hpp): forward-mode sweeps of the RNEA recursion, one
 * differentiated joint at a time, each column stored as it completes; fd_deriv evaluates the
 * bias, H and L D L^T once and back-substitutes every column through the kept factors.
 *
 * Input domain: as above -- a configuration with a NaN / Inf input or an angle past the bound gets
 * NaN in every element of every output; the others are unaffected.
 *
 * Accuracy (tests/test_deriv_host.py, tests/test_gpu_deriv.py; reference: Richardson-extrapolated
 * central differences of the fp64 oracle, self-consistent to 1e-10).  fp64: dtau_dq, dtau_dqd
 * |d| <= 1e-8 (1 + |ref|) element-wise; the forward-dynamics matrices satisfy
 * sym(H) dqdd_dtau = I to 1e-9 and sym(H) dqdd_dq + dtau_dq = 0 to 1e-8, scaled.  fp32 (FR3, over
 * its limits, measured): dtau_dq, dtau_dqd per column max_i |d_ik| <= 1e-4 (1 + max_i |ref_ik|)
 * (measured 2.2e-6); the forward-dynamics matrices X as row-sum residuals
 * |H_s X + dtau_dq| <= 60 eps32 (|H_s| |X| + |dtau_dq|) (measured constant 14.8, below the 24 of the
 * fp32 forward-dynamics contract above). */
int multibody_rnea_deriv_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                   float *dtau_dq, float *dtau_dqd, int64_t batch, int64_t ld, void *stream);
int multibody_rnea_deriv_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                   double *dtau_dq, double *dtau_dqd, int64_t batch, int64_t ld, void *stream);
int multibody_fd_deriv_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *tau, float *qdd_out,
                                 float *dqdd_dq, float *dqdd_dqd, float *dqdd_dtau, int64_t batch, int64_t ld,
                                 void *stream);
int multibody_fd_deriv_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                                 double *qdd_out, double *dqdd_dq, double *dqdd_dqd, double *dqdd_dtau, int64_t batch,
                                 int64_t ld, void *stream);
/* Blocking host-pointer forms: [n][batch] inputs, [n * n][batch] matrices ([n][batch] qdd_out). */
int multibody_rnea_deriv_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                        float *dtau_dq, float *dtau_dqd, int64_t batch);
int multibody_rnea_deriv_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                        double *dtau_dq, double *dtau_dqd, int64_t batch);
int multibody_fd_deriv_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *tau,
                                      float *qdd_out, float *dqdd_dq, float *dqdd_dqd, float *dqdd_dtau,
                                      int64_t batch);
int multibody_fd_deriv_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                                      double *qdd_out, double *dqdd_dq, double *dqdd_dqd, double *dqdd_dtau,
                                      int64_t batch);
/* One configuration, fp64, caller-provided buffers (n * n doubles per matrix, n for qdd), on the
 * calling thread: the same lane body compiled for the host, no GPU needed (an FMA3 / AVX2 CPU
 * and a chain length of multibody_supported_dofs, else RB_ERR_UNSUPPORTED). */
int multibody_rnea_deriv(const Multibody *mb, const double *q, const double *qd, const double *qdd, double *dtau_dq,
                         double *dtau_dqd);
int multibody_fd_deriv(const Multibody *mb, const double *q, const double *qd, const double *tau, double *qdd,
                       double *dqdd_dq, double *dqdd_dqd, double *dqdd_dtau);

/* ---- reverse-mode gradient of the fused rollout -------------------------------- */
/* The vector-Jacobian product of K rollout steps (multibody_rollout_batch_*), for gradient-based
 * shooting.  Step k reads the state (q_k, v_k) and tau_k:
 *   a_k = fd(q_k, v_k, tau_k)     v_{k+1} = v_k + dt a_k     q_{k+1} = q_k + dt v_{k+1}
 * Inputs: the initial state q, qd, the torques tau_seq, and cotangents gq[k], gqd[k] of the state
 * after step k, k = 0 .. K-1 -- gq[k] pairs with traj[k] of the rollout, gqd[k] with the velocity at
 * the same instant (gqd[K-1] with the final qd).  Outputs: the gradient of
 *   L = sum_k gq[k] . q_{k+1} + gqd[k] . v_{k+1}
 * with respect to the initial state (g_q0, g_qd0) and every torque (g_tau), the size of the inputs;
 * no Jacobian matrix is formed or stored.  One launch: the trajectory is recomputed forward, each
 * pre-step state parked in `work`, then the adjoint recursion runs backward (one forward-dynamics
 * factorisation, two solves and the tangent column sweeps of multibody_fd_deriv_batch_* per step,
 * each column dotted with the adjoint as it completes; rollout_vjp_body.hip.hpp).
 *
 * Layout: q, qd, g_q0, g_qd0 are [n][ld]; tau_seq, gq, gqd, g_tau are [K][n][ld] (step k, joint j,
 * configuration b at (k*n + j)*ld + b, as the rollout's tau_seq); work is [K][2n][ld] of scratch
 * the caller provides, its contents on return unspecified.  Every array is required.  Checks, in
 * order: handle, batch >= 0, ld >= batch, batch == 0 (RB_OK, nothing else looked at), K < 0
 * ("negative step count") or K == 0 (nothing to differentiate) RB_ERR_ARG, a NULL array RB_ERR_NULL,
 * an output or the workspace that is also an input or passed twice RB_ERR_ARG, then the scope.
 * Batches are split at 2^28 per launch.
 *
 * Scope: as multibody_fd_deriv_batch_* -- serial revolute chains (z-axis or
 * RB_MODEL_GENERAL_AXES) on the mass-matrix forward dynamics, up to 12 links; anything else returns
 * RB_ERR_UNSUPPORTED and rb_last_error() names the condition.  A model-specialised (hipRTC) kernel
 * only: with hipRTC disabled or failed RB_ERR_UNSUPPORTED with the log.  SoA rows only.
 *
 * Relation to multibody_rollout_batch_*: the trajectory differentiated is the rollout of the
 * mass-matrix forward dynamics.  For chains of 9 to 12 links multibody_rollout_batch_* integrates
 * the articulated-body form instead, so the two trajectories agree to rounding, not bit for bit.
 *
 * Input domain: q_k, v_k and tau_k are checked at every step; a configuration that leaves the domain
 * at any step (a NaN / Inf input, an angle past the bound, also one the integration runs into) gets
 * NaN in every element of g_q0, g_qd0 and g_tau, the others are unaffected.  The cotangents gq, gqd
 * are NOT checked: a NaN there propagates by arithmetic into the outputs it reaches.
 *
 * Accuracy (tests/test_rollout_vjp_host.py, tests/test_gpu_rollout_vjp.py; reference: Richardson
 * central differences of the fp64 oracle's own rollout along a random direction): fp64
 * |<g, d> - ref| <= 1e-7 (1 + |ref|) wherever that reference is self-consistent to 1e-8 (measured
 * 2e-12 FR3, 2e-11 on 12 links, K = 3); the kernel agrees with the host form of the same lane body to
 * 1.02e-13 relative (measured 1.02e-14, K = 3).  fp32 against the fp64 kernel on the same
 * fp32-rounded inputs (B = 257, K = 3, dt = 0.01), per output array and configuration:
 * max|d| <= 4e-4 (1 + max|ref|) (measured 5.1e-6 FR3, 9.7e-5 on 12 links). */
int multibody_rollout_vjp_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *tau_seq,
                                    double dt, int K, const float *gq, const float *gqd, float *g_q0, float *g_qd0,
                                    float *g_tau, float *work, int64_t batch, int64_t ld, void *stream);
int multibody_rollout_vjp_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *tau_seq,
                                    double dt, int K, const double *gq, const double *gqd, double *g_q0, double *g_qd0,
                                    double *g_tau, double *work, int64_t batch, int64_t ld, void *stream);
/* Blocking host-pointer forms: contiguous host arrays (ld = batch); the workspace is internal. */
int multibody_rollout_vjp_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *tau_seq,
                                         double dt, int K, const float *gq, const float *gqd, float *g_q0,
                                         float *g_qd0, float *g_tau, int64_t batch);
int multibody_rollout_vjp_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *tau_seq,
                                         double dt, int K, const double *gq, const double *gqd, double *g_q0,
                                         double *g_qd0, double *g_tau, int64_t batch);
/* One configuration, fp64, [K][n] arrays, on the calling thread: the same lane body compiled for
 * the host, its workspace internal (an FMA3 / AVX2 CPU, else RB_ERR_UNSUPPORTED). */
int multibody_rollout_vjp(const Multibody *mb, const double *q, const double *qd, const double *tau_seq, double dt,
                          int K, const double *gq, const double *gqd, double *g_q0, double *g_qd0, double *g_tau);
/* Inspection of that kernel (it has no kind number in the multibody_*_ex queries above): the
 * generated source / the hipRTC compile for `arch` of the kernel a launch of `batch`
 * configurations runs, as multibody_jit_source_ex / multibody_jit_compile_ex; a model out of scope
 * has the empty source and -RB_ERR_UNSUPPORTED. */
int multibody_rollout_vjp_jit_source(const Multibody *mb, int f64, int64_t batch, char *buf, int64_t cap);
int64_t multibody_rollout_vjp_jit_compile(const Multibody *mb, int f64, int64_t batch, const char *arch);

/* ---- external link wrenches ----------------------------------------------------- */
/* Inverse and forward dynamics with one external spatial wrench per moving link and configuration
 * (contact forces, payloads, end-effector loads, thrusters):
 *   tau = rnea_ext(q, qd, qdd, fext) = rnea(q, qd, qdd) - sum_j J_j(q)^T fext_j
 *   qdd = fd_ext(q, qd, tau, fext)   = fd(q, qd, tau + sum_j J_j(q)^T fext_j)
 * J_j is the body Jacobian of link j and fext_j the wrench acting ON link j.
 *
 * Frame: fext_j is expressed in link j's own URDF link frame -- the joint's child frame, after the
 * joint's motion, the frame multibody_fwd_kin / multibody_jac report for the last link -- and
 * applied at that frame's origin.  With RB_MODEL_GENERAL_AXES (and the tree reading) the kernels
 * rotate it into their own per-link frame; a caller never sees that frame.
 *
 * Layout: fext is [6 n][ld]; component c of link j for configuration b at fext[(6 j + c) * ld + b],
 * c = 0..2 the force, c = 3..5 the moment -- the [lin; rot] row order of the Jacobian.  So for a
 * wrench f on the last link only, rnea - rnea_ext = J^T f with J what multibody_jac_batch_* returns.
 * The six virtual links of a floating base have rows like any other link.  q, qd, qdd, tau are
 * [n][ld].  fext is required: a caller without forces uses multibody_rnea_batch_* / _fd_batch_*.
 * The single-configuration forms take fext as [6 n].
 *
 * Algorithm (ext_body.hip.hpp; Featherstone 2008): the wrench enters where each link's force is
 * formed, f_j = I_j a_j + v_j x* I_j v_j - fext_j (Table 5.1) and pA_j = v_j x* I_j v_j - fext_j
 * (Table 7.1), from rows loaded at link j's forward step.  fd_ext takes the formulation
 * multibody_fd_batch_* takes for the model: the mass-matrix form for serial chains up to 12 links,
 * with the bias C = rnea_ext(q, qd, 0, fext), else the articulated-body algorithm.
 *
 * Scope: every model the model-specialised kernels run -- serial chains under the reference's
 * reading or with general axes, of every supported length; kinematic trees; prismatic joints; a
 * floating base.  Model-specialised (hipRTC) kernels only, no kind number: with hipRTC disabled or
 * failed RB_ERR_UNSUPPORTED with the log.  SoA rows only (no tiled form), one configuration per
 * lane, batches split at 2^28 per launch.
 *
 * Checks, in order: handle (RB_ERR_NULL), batch >= 0, ld >= batch (RB_ERR_ARG), batch == 0 (RB_OK,
 * nothing else looked at), a NULL array (RB_ERR_NULL), the output passed as one of the inputs
 * (RB_ERR_ARG; the device-pointer and single-configuration forms), then hipRTC.
 *
 * Input domain: as above, every fext component a value like qd: a configuration with a NaN / Inf in
 * any input or an angle past the bound gets NaN in every output, the others are unaffected.
 *
 * Accuracy (tests/test_ext_host.py, tests/test_gpu_ext.py; reference: the fp64 oracle's rnea / fd
 * with J^T f composed link by link from its own transforms).  fp64: tau |d| <= 1e-9 (1 + |ref|);
 * fd_ext residual |rnea(q, qd, qdd) - (tau + J^T f)| <= 1e-8 (1 + |tau + J^T f|) and qdd to
 * 1e-7 (1 + |ref|); zero wrenches agree with the plain entry points to 1e-12 (1 + |ref|).  fp32
 * against the fp64 kernel on the same fp32-rounded inputs, per configuration: rnea_ext
 * max|d| <= 1e-4 (1 + max|ref|), fd_ext residual norm-wise <= 1e-3.  Measured (MI355X, B = 257,
 * forces +-20 N, moments +-5 N m): fp64 tau 2.0e-14 FR3 / 1.6e-13 16 links / 1.0e-13 floating base;
 * fd_ext residual 4.3e-12 and qdd 6.0e-11 at most (16 links); zero wrench 2.8e-13 at most; fp32
 * rnea_ext 8.3e-7 (floating base), fd_ext residual 7.9e-6 (FR3). */
int multibody_rnea_ext_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                 const float *fext, float *tau, int64_t batch, int64_t ld, void *stream);
int multibody_rnea_ext_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                 const double *fext, double *tau, int64_t batch, int64_t ld, void *stream);
int multibody_fd_ext_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *tau,
                               const float *fext, float *qdd, int64_t batch, int64_t ld, void *stream);
int multibody_fd_ext_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                               const double *fext, double *qdd, int64_t batch, int64_t ld, void *stream);
/* Blocking host-pointer forms: contiguous host arrays (ld = batch). */
int multibody_rnea_ext_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                      const float *fext, float *tau, int64_t batch);
int multibody_rnea_ext_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                      const double *fext, double *tau, int64_t batch);
int multibody_fd_ext_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *tau,
                                    const float *fext, float *qdd, int64_t batch);
int multibody_fd_ext_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                                    const double *fext, double *qdd, int64_t batch);
/* One configuration, fp64, caller-provided output of n doubles, on the calling thread: the same
 * lane body compiled for the host, no GPU needed.  Serial revolute chains of a
 * multibody_supported_dofs length on an FMA3 / AVX2 CPU; anything else (trees, prismatic joints, a
 * floating base) RB_ERR_UNSUPPORTED.  fd_ext: the mass-matrix form up to 12 links, else the ABA. */
int multibody_rnea_ext(const Multibody *mb, const double *q, const double *qd, const double *qdd, const double *fext,
                       double *tau);
int multibody_fd_ext(const Multibody *mb, const double *q, const double *qd, const double *tau, const double *fext,
                     double *qdd);
/* Inspection of those kernels (no kind number): fd != 0 selects fd_ext, else rnea_ext; otherwise as
 * multibody_rollout_vjp_jit_source / _compile. */
int multibody_ext_jit_source(const Multibody *mb, int fd, int f64, int64_t batch, char *buf, int64_t cap);
int64_t multibody_ext_jit_compile(const Multibody *mb, int fd, int f64, int64_t batch, const char *arch);

/* ---- kinematics of every link --------------------------------------------------- */
/* Pose and spatial velocity of EVERY link (multibody_fwd_kin / multibody_jac answer for the last
 * link only, and without an orientation): what a caller needs to form the wrenches fext of the
 * entry points above -- where a foot's frame is, how it is oriented, how fast its origin moves.
 *
 * Frame: link j's own URDF link frame -- the joint's child frame, after the joint's motion; the
 * frame fext_j is given in, and the frame multibody_fwd_kin / multibody_jac report for the last
 * link.  With RB_MODEL_GENERAL_AXES (and the tree reading) the kernels sweep in their own per-link
 * frames and turn the results on the way out; a caller never sees that frame.
 *
 * Layout (SoA rows of leading dimension ld, configuration b):
 *   pos [3 n][ld]  pos[(3 j + c) * ld + b]: component c of the frame origin, in the base frame
 *   rot [9 n][ld]  rot[(9 j + e) * ld + b], e = row + 3 * col (column-major, the ABI's order): the
 *                  rotation R_j with x_base = R_j x_link
 *   vel [6 n][ld]  rows 6 j + 0..2 the linear velocity of the frame origin, rows 6 j + 3..5 the
 *                  angular velocity, both expressed in link j's frame -- the [lin; rot] row order of
 *                  the Jacobian and of fext: vel_j = J_j(q) qd with J_j the body Jacobian of link j,
 *                  so sum_j fext_j . vel_j is the power the wrenches deliver.  Purely kinematic: the
 *                  reference's gravity-as-base-acceleration does not enter.
 * q, qd are [n][ld].  The six virtual links of a floating base have rows like any other link.  The
 * single-configuration forms take pos [3 n], rot [9 n], vel [6 n].
 *
 * Algorithm (link_kin_body.hip.hpp): one root-to-leaf sweep, one configuration per lane; a link's
 * rows are stored as soon as the link completes.  Only a link with more than one child is kept
 * beyond the next step of the sweep (a serial chain keeps one pose / velocity, a quadruped its
 * trunk's too).
 *
 * Scope: every model the model-specialised kernels run -- serial chains under the reference's
 * reading or with general axes, of every supported length; kinematic trees; prismatic joints; a
 * floating base.  Model-specialised (hipRTC) kernels only, no kind number: with hipRTC disabled or
 * failed RB_ERR_UNSUPPORTED with the log.  SoA rows only (no tiled form), batches split at 2^28
 * per launch.
 *
 * Checks, in order: handle (RB_ERR_NULL), batch >= 0, ld >= batch (RB_ERR_ARG), batch == 0 (RB_OK,
 * nothing else looked at), a NULL array (RB_ERR_NULL; every array is required), an output passed as
 * one of the inputs or as the other output (RB_ERR_ARG), then hipRTC.
 *
 * Input domain: as above: a configuration with a NaN / Inf in q or qd, or an angle past the bound,
 * gets NaN in every element of every output; the others are unaffected.  Every input is checked
 * before the configuration's first row is stored.
 *
 * Accuracy (tests/test_link_kin_host.py, tests/test_gpu_link_kin.py; reference tests/link_kin_ref.py:
 * world poses accumulated root to leaf from the 6x6 Featherstone model's own joint transforms,
 * velocities from v_j = X_j v_parent + S_j qd_j).  fp64: every element of pos, rot, vel
 * |d| <= 1e-9 (1 + |ref|), the fwd_kin / jac contract; the last link's pos / vel agree with
 * multibody_fwd_kin / multibody_jac . qd to 1e-12 (1 + |ref|); rot is orthonormal to 1e-12; and
 * sum_j fext_j . vel_j = qd . (rnea - rnea_ext) to 1e-8 (1 + sum_j |fext_j . vel_j|).  fp32 against
 * the fp64 kernel on the same fp32-rounded inputs, per configuration and output array:
 * max|d| <= 1e-4 (1 + max|ref|).  Measured (MI355X, B = 257): fp64 9.3e-16 FR3 / 2.1e-15 16 links /
 * 1.8e-15 five links with general axes / 1.8e-15 the 9-joint tree / 2.6e-15 floating base; the
 * power identity 1.1e-15 at most; |q| ~ 2^40 rad 1.4e-15; fp32 2.7e-7 at most (floating base, vel).
 * Single-configuration forms on the host: 4.8e-16 FR3, 4.1e-15 at most (30 links). */
int multibody_link_pose_batch_f32(const Multibody *mb, const float *q, float *pos, float *rot, int64_t batch,
                                  int64_t ld, void *stream);
int multibody_link_pose_batch_f64(const Multibody *mb, const double *q, double *pos, double *rot, int64_t batch,
                                  int64_t ld, void *stream);
int multibody_link_vel_batch_f32(const Multibody *mb, const float *q, const float *qd, float *vel, int64_t batch,
                                 int64_t ld, void *stream);
int multibody_link_vel_batch_f64(const Multibody *mb, const double *q, const double *qd, double *vel, int64_t batch,
                                 int64_t ld, void *stream);
/* Blocking host-pointer forms: contiguous host arrays (ld = batch). */
int multibody_link_pose_batch_host_f32(const Multibody *mb, const float *q, float *pos, float *rot, int64_t batch);
int multibody_link_pose_batch_host_f64(const Multibody *mb, const double *q, double *pos, double *rot, int64_t batch);
int multibody_link_vel_batch_host_f32(const Multibody *mb, const float *q, const float *qd, float *vel, int64_t batch);
int multibody_link_vel_batch_host_f64(const Multibody *mb, const double *q, const double *qd, double *vel,
                                      int64_t batch);
/* One configuration, fp64, caller-provided outputs, on the calling thread: the same lane body
 * compiled for the host, no GPU needed.  Serial revolute chains of a multibody_supported_dofs length
 * on an FMA3 / AVX2 CPU; anything else (trees, prismatic joints, a floating base)
 * RB_ERR_UNSUPPORTED -- the scope of multibody_rnea_ext. */
int multibody_link_pose(const Multibody *mb, const double *q, double *pos, double *rot);
int multibody_link_vel(const Multibody *mb, const double *q, const double *qd, double *vel);
/* Inspection of those kernels (no kind number): vel != 0 selects link_vel, else link_pose; otherwise
 * as multibody_ext_jit_source / _compile. */
int multibody_link_kin_jit_source(const Multibody *mb, int vel, int f64, int64_t batch, char *buf, int64_t cap);
int64_t multibody_link_kin_jit_compile(const Multibody *mb, int vel, int f64, int64_t batch, const char *arch);

/* ---- centre of mass, centroidal momentum, energy ---------------------------------- */
/* The whole-body quantities costs and constraints of legged robots are written in, reduced on chip:
 * 3 - 11 rows per configuration (6 n for the momentum matrix) instead of the 18 n rows of
 * multibody_link_pose / _vel and a reduction in the caller's code.
 *
 * Definitions.  pos_j, R_j, lin_j, ang_j are what multibody_link_pose / multibody_link_vel define
 * (URDF link frame of link j); m_j, c_j, Ic_j the mass, the centre of mass in that frame and the
 * rotational inertia about c_j in that frame's axes, all after fixed-joint merging;
 * M = multibody_total_mass(mb); g = 9.81.
 *   x_j   = pos_j + R_j c_j                          link COM, base frame
 *   xd_j  = R_j (lin_j + ang_j x c_j)                its velocity, base frame
 *   com   = (1/M) sum_j m_j x_j
 *   l     = sum_j m_j xd_j                           linear momentum (= M d com/dt)
 *   k     = sum_j [ R_j (Ic_j ang_j) + m_j (x_j - com) x xd_j ]   angular momentum about com, base axes
 *   hg    = [ l ; k ]                                [lin; ang], the ABI's row order
 *   T     = 1/2 sum_j ( m_j |xd_j|^2 + ang_j . Ic_j ang_j )       = 1/2 qd^T sym(H) qd, H of multibody_crba
 *   U     = g M com_z                                so that dU/dq = rnea(q, 0, 0)
 *   A_G(q): the 6 x n centroidal momentum matrix, hg = A_G(q) qd for every qd; rows 0..2 / M are
 *           the COM Jacobian
 * Gravity is the reference's +9.81 base acceleration along base z, as everywhere in this ABI.  The
 * six virtual links of a floating base are massless and count like any other link.
 *
 * Layout (SoA rows of leading dimension ld, configuration b; q, qd are [n][ld]):
 *   com    [3][ld]    com[c * ld + b]
 *   hg     [6][ld]    rows 0..2 l, rows 3..5 k
 *   energy [2][ld]    row 0 T, row 1 U
 *   ag     [6 n][ld]  ag[e * ld + b], e = row + 6 * col (column-major, the order of multibody_jac)
 * The single-configuration forms take com [3], hg [6], energy [2], ag [6 n].
 *
 * Algorithm (centroidal_body.hip.hpp).  com / centroidal: one root-to-leaf sweep, one configuration
 * per lane, carrying the world pose (and link velocity) of the current link and of links with more
 * than one child only; a link adds m_j x_j, its momentum about the base origin and its energy to
 * accumulators and is forgotten; k is shifted to com once at the end.  cmm: the forward sweep leaves
 * each link's joint axis, origin and ten inertial numbers about the base origin in base coordinates,
 * a leaf-to-root sweep sums them into subtree composites, and column k -- the momentum of subtree k
 * under the unit motion of joint k, shifted to com -- is stored as it completes.
 *
 * Scope: every model the link-kinematics kernels run -- serial chains under either reading and of
 * every supported length, general axes, kinematic trees, prismatic joints, a floating base -- with
 * M > 0 (else RB_ERR_UNSUPPORTED).  Model-specialised (hipRTC) kernels only, no kind number: with
 * hipRTC disabled or failed RB_ERR_UNSUPPORTED with the log.  SoA rows only (no tiled form), batches
 * split at 2^28 per launch.
 *
 * Checks, in order: handle (RB_ERR_NULL), batch >= 0, ld >= batch (RB_ERR_ARG), batch == 0 (RB_OK,
 * nothing else looked at), a NULL array (RB_ERR_NULL; every array is required), an output passed as
 * one of the inputs or as another output (RB_ERR_ARG), a model without mass (RB_ERR_UNSUPPORTED),
 * then hipRTC.
 *
 * Input domain: as above: a configuration with a NaN / Inf in q or qd, or an angle past the bound,
 * gets NaN in every element of every output; the others are unaffected.  Every input is checked
 * before the configuration's first row is stored.
 *
 * Accuracy (tests/test_centroidal_host.py, tests/test_gpu_centroidal.py; reference
 * tests/centroidal_ref.py: the definitions above evaluated with the 6x6 Featherstone model's joint
 * transforms and link inertias, A_G column k as hg at qd = e_k).  fp64: every element of every output
 * |d| <= 1e-9 (1 + |ref|); hg = A_G qd, T = 1/2 qd^T sym(H) qd with H of multibody_crba and
 * U = g M com_z to 1e-12 scaled; A_G[0:3]^T (0, 0, g) = rnea(q, 0, 0) to 1e-9 scaled; a floating
 * base's three translation columns of A_G are [M 1; 0] to 1e-12 scaled.  fp32 against the fp64
 * kernel on the same fp32-rounded inputs, per configuration and output array:
 * max|d| <= 1e-4 (1 + max|ref|).
 * Measured (MI355X, B = 257): fp64 against the reference 1.4e-15 FR3 / 2.2e-14 16 links / 6.3e-15
 * five links with general axes / 1.9e-15 the 9-joint tree / 1.2e-14 floating base (the largest is energy or
 * hg each time, com 3.4e-16 at most); hg = A_G qd 2.0e-14 at most (floating base), T against crba 3.4e-15,
 * the gravity identity 9.4e-14 (16 links), U bit for bit, the translation columns 9.9e-15; kernel against
 * the host form 2.2e-15; fp32 1.2e-6 at most (general axes, energy).  Single-configuration forms on the
 * host: 1.4e-15 FR3, 1.7e-14 at most (30 links). */
int multibody_com_batch_f32(const Multibody *mb, const float *q, float *com, int64_t batch, int64_t ld, void *stream);
int multibody_com_batch_f64(const Multibody *mb, const double *q, double *com, int64_t batch, int64_t ld,
                            void *stream);
int multibody_centroidal_batch_f32(const Multibody *mb, const float *q, const float *qd, float *com, float *hg,
                                   float *energy, int64_t batch, int64_t ld, void *stream);
int multibody_centroidal_batch_f64(const Multibody *mb, const double *q, const double *qd, double *com, double *hg,
                                   double *energy, int64_t batch, int64_t ld, void *stream);
int multibody_cmm_batch_f32(const Multibody *mb, const float *q, float *ag, int64_t batch, int64_t ld, void *stream);
int multibody_cmm_batch_f64(const Multibody *mb, const double *q, double *ag, int64_t batch, int64_t ld,
                            void *stream);
/* Blocking host-pointer forms: contiguous host arrays (ld = batch). */
int multibody_com_batch_host_f32(const Multibody *mb, const float *q, float *com, int64_t batch);
int multibody_com_batch_host_f64(const Multibody *mb, const double *q, double *com, int64_t batch);
int multibody_centroidal_batch_host_f32(const Multibody *mb, const float *q, const float *qd, float *com, float *hg,
                                        float *energy, int64_t batch);
int multibody_centroidal_batch_host_f64(const Multibody *mb, const double *q, const double *qd, double *com,
                                        double *hg, double *energy, int64_t batch);
int multibody_cmm_batch_host_f32(const Multibody *mb, const float *q, float *ag, int64_t batch);
int multibody_cmm_batch_host_f64(const Multibody *mb, const double *q, double *ag, int64_t batch);
/* One configuration, fp64, caller-provided outputs, on the calling thread: the same lane body
 * compiled for the host, no GPU needed.  The scope of multibody_link_pose: serial revolute chains of
 * a multibody_supported_dofs length on an FMA3 / AVX2 CPU; anything else RB_ERR_UNSUPPORTED. */
int multibody_com(const Multibody *mb, const double *q, double *com);
int multibody_centroidal(const Multibody *mb, const double *q, const double *qd, double *com, double *hg,
                         double *energy);
int multibody_cmm(const Multibody *mb, const double *q, double *ag);
/* Inspection of those kernels (no kind number): which = 0 com, 1 centroidal, 2 cmm (anything else
 * RB_ERR_ARG); otherwise as multibody_link_kin_jit_source / _compile. */
int multibody_centroidal_jit_source(const Multibody *mb, int which, int f64, int64_t batch, char *buf, int64_t cap);
int64_t multibody_centroidal_jit_compile(const Multibody *mb, int which, int f64, int64_t batch, const char *arch);

/* ---- compliant ground contact ---------------------------------------------------- */
/* The step between the link kinematics and the external wrenches: a contact model that maps
 * (q, qd) to fext, and a fused K-step rollout that evaluates it on chip at every step and
 * integrates fd_ext under it (one launch; a step moves the step's tau and its traj row through
 * memory and nothing else).
 *
 * A contact set belongs to a model.  It holds P points, 1 <= P <= RB_CONTACT_MAX_POINTS, each with a
 * moving-link index l_p in 0 .. n-1 (the numbering of multibody_topology; the six virtual links of a
 * floating base count like any other) and a position c_p in that link's URDF link frame; one plane
 * in the base frame, a unit normal nhat and an offset d, the free side nhat . x > d; and four law
 * parameters: stiffness k >= 0 [N/m], damping c >= 0 [s/m], friction mu >= 0, slip velocity
 * v_s > 0 [m/s].  Several points may sit on one link.
 *
 * The law.  For a state (q, v), with pos_j, R_j, vel_j = [lin_j; ang_j] exactly as
 * multibody_link_pose / multibody_link_vel define them:
 *
 *   x_p   = pos_l + R_l c_p                          point in the base frame
 *   xd_p  = R_l (lin_l + ang_l x c_p)                its velocity in the base frame
 *   phi   = max(d - nhat . x_p, 0)                   penetration depth
 *   phid  = -nhat . xd_p                             penetration rate
 *   f_n   = max(k * phi * (1 + c * phid), 0)         Hunt-Crossley normal force, never adhesive
 *   v_t   = xd_p + phid * nhat                       tangential velocity
 *   F_p   = f_n * nhat - mu * f_n * v_t / sqrt(v_t . v_t + v_s^2)
 *   g_p   = R_l^T F_p                                the force in the link frame
 *   fext_l += [ g_p ; c_p x g_p ]                    [force; moment], the ABI's fext row order
 *
 * Every piece is continuous in the state: the normal force goes to zero with the depth, the
 * friction is regularised by v_s.  Rows of links with no point are exact zeros.
 *
 * The fused rollout does, at step k:
 *
 *   fext     = contact(q_k, v_k)
 *   a_k      = fd_ext(q_k, v_k, tau_k, fext)
 *   v_{k+1}  = v_k + dt a_k
 *   q_{k+1}  = q_k + dt v_{k+1}
 *   traj[k]  = q_{k+1}
 *
 * -- multibody_rollout_batch's integrator and fused-multiply-add order.  It is an explicit penalty
 * method: stability needs roughly dt * sqrt(k / m_link) < 1, which is the caller's responsibility.
 *
 * The set rides on the handle: multibody_with_contacts returns a NEW immutable handle, the same
 * model plus the set (mb is not modified; free both).  The set is model data and is compiled into
 * the kernels like the rest of the model, so a link without a point costs nothing and mu == 0 drops
 * the friction -- and changing a stiffness is a different model that compiles its own kernels.
 * multibody_export_blob / multibody_new_from_blob carry the set; the blob of a model without one is
 * what it was.  multibody_with_contacts returns NULL (rb_last_error names the field) for n_points
 * outside 1..16, a link index outside 0..n-1, any non-finite value, | |normal| - 1 | > 1e-6, a
 * negative stiffness, damping or friction, slip_velocity <= 0.
 *
 * Layout: q, qd [n][ld]; fext [6 n][ld] as multibody_rnea_ext takes it; cforce [3 P][ld], F_p in the
 * base frame at row 3 p + c; tau_seq, traj [K n][ld] as multibody_rollout_batch; q and qd of the
 * rollout are overwritten with the final state.  Every array is required, traj and cforce included.
 *
 * Checks, in order: handle (RB_ERR_NULL), batch >= 0, ld >= batch (RB_ERR_ARG), the rollout's K < 0
 * (RB_ERR_ARG "negative step count"), batch == 0 or the rollout's K == 0 (RB_OK, nothing else looked
 * at), a NULL array (RB_ERR_NULL), an output -- the rollout's q and qd included -- that is also an
 * input or another output (RB_ERR_ARG), a model without a contact set (RB_ERR_UNSUPPORTED, naming
 * multibody_with_contacts), then hipRTC.
 *
 * Scope: every model the external-wrench kernels run.  Model-specialised (hipRTC) kernels only, one
 * configuration per lane, SoA rows, no kind number, batches split at 2^28.  The rollout's forward
 * dynamics is the formulation multibody_rollout_batch takes for the model.
 *
 * Input domain: as above; a configuration with a NaN / Inf input or an angle past the bound gets NaN
 * in every output, the others are unaffected.  The rollout checks the state and tau_k at every
 * step: everything from the first bad step on is NaN.
 *
 * Accuracy (tests/test_contact_host.py, tests/test_gpu_contact.py; reference tests/contact_ref.py,
 * the law above on tests/link_kin_ref.py and the oracle's forward dynamics).  fp64: fext, cforce
 * |d| <= 1e-9 (1 + |ref|); traj and the final state 1e-7 (1 + |ref|), against the reference and
 * against the composed contact_wrench / fd_ext / update sequence; the power identity
 * sum_p F_p . xd_p = sum_j fext_j . vel_j to 1e-8 scaled.  fp32 against the fp64 kernel on the same
 * fp32-rounded inputs, per configuration and array: contact_wrench max|d| <= 1e-4 (1 + max|ref|);
 * rollout_contact (K = 4, dt = 1e-3) traj and final state 4e-4 (1 + max|ref|) -- 8x the measured
 * maximum, 4.7e-5 (the 16-link chain's final qd).  Measured (MI355X, B = 257, about half the points
 * in contact): fp64 wrench 6.2e-13 at most; fused rollout against the composition 2.8e-14, against
 * the reference 1.3e-13; fp32 wrench 1.7e-5 FR3 / 7.1e-5 16 links / 1.0e-5 at most the others; fp32
 * rollout traj 6.4e-6 at most, final qd 4.7e-5 at most.  Single-configuration forms on the host:
 * wrench 1.4e-12 at most (30 links), rollout (K = 3) 1.4e-11. */
enum { RB_CONTACT_MAX_POINTS = 16 };
typedef struct {
    int n_points;
    int link[RB_CONTACT_MAX_POINTS];
    double point[RB_CONTACT_MAX_POINTS][3];
    double normal[3];
    double offset;
    double stiffness, damping, friction, slip_velocity;
} rb_contact_model;

/* A NEW immutable handle: the same model plus the contact set.  mb is not modified. */
Multibody *multibody_with_contacts(const Multibody *mb, const rb_contact_model *cm);
/* Returns n_points (0: the model carries no contact set); fills *out when non-NULL. */
int multibody_contact_model(const Multibody *mb, rb_contact_model *out);

int multibody_contact_wrench_batch_f32(const Multibody *mb, const float *q, const float *qd, float *fext,
                                       float *cforce, int64_t batch, int64_t ld, void *stream);
int multibody_contact_wrench_batch_f64(const Multibody *mb, const double *q, const double *qd, double *fext,
                                       double *cforce, int64_t batch, int64_t ld, void *stream);
int multibody_rollout_contact_batch_f32(const Multibody *mb, float *q, float *qd, const float *tau_seq, double dt,
                                        int K, float *traj, int64_t batch, int64_t ld, void *stream);
int multibody_rollout_contact_batch_f64(const Multibody *mb, double *q, double *qd, const double *tau_seq, double dt,
                                        int K, double *traj, int64_t batch, int64_t ld, void *stream);
/* Blocking host-pointer forms: contiguous host arrays (ld = batch). */
int multibody_contact_wrench_batch_host_f32(const Multibody *mb, const float *q, const float *qd, float *fext,
                                            float *cforce, int64_t batch);
int multibody_contact_wrench_batch_host_f64(const Multibody *mb, const double *q, const double *qd, double *fext,
                                            double *cforce, int64_t batch);
int multibody_rollout_contact_batch_host_f32(const Multibody *mb, float *q, float *qd, const float *tau_seq, double dt,
                                             int K, float *traj, int64_t batch);
int multibody_rollout_contact_batch_host_f64(const Multibody *mb, double *q, double *qd, const double *tau_seq,
                                             double dt, int K, double *traj, int64_t batch);
/* One configuration, fp64, on the calling thread: the scope of multibody_rnea_ext (serial revolute
 * chains of a multibody_supported_dofs length on an FMA3 / AVX2 CPU). */
int multibody_contact_wrench(const Multibody *mb, const double *q, const double *qd, double *fext, double *cforce);
int multibody_rollout_contact(const Multibody *mb, double *q, double *qd, const double *tau_seq, double dt, int K,
                              double *traj);
/* Inspection of those kernels (no kind number): rollout != 0 selects rollout_contact, else
 * contact_wrench; a model without a contact set has the empty source / -RB_ERR_UNSUPPORTED;
 * otherwise as multibody_ext_jit_source / _compile. */
int multibody_contact_jit_source(const Multibody *mb, int rollout, int f64, int64_t batch, char *buf, int64_t cap);
int64_t multibody_contact_jit_compile(const Multibody *mb, int rollout, int f64, int64_t batch, const char *arch);

/* ---- reverse-mode gradient of the fused contact rollout --------------------------- */
/* multibody_rollout_vjp_* for a handle that carries a contact set: the vector-Jacobian product of
 * K steps of multibody_rollout_contact_batch_* on the mass-matrix forward dynamics, one launch.
 *   fext_k = contact(q_k, v_k)            (the law above, unchanged)
 *   a_k = fd_ext(q_k, v_k, tau_k, fext_k)     v_{k+1} = v_k + dt a_k     q_{k+1} = q_k + dt v_{k+1}
 *   L = sum_k gq[k] . q_{k+1} + gqd[k] . v_{k+1}
 * Arguments, layout, cotangent convention, outputs (g_q0, g_qd0, g_tau) and the workspace
 * (work [K][2n][ld]) are those of multibody_rollout_vjp_batch_*, argument for argument.
 *
 * Law of the derivative.  With T(q, v, a) = rnea(q, v, a) - sum_j J_j(q)^T fext_j(q, v), the adjoint
 * step of multibody_rollout_vjp_* runs with rnea replaced by T (total derivatives in q and v, a_k
 * held).  The law is continuous and piecewise smooth; its two max(., 0) take the derivative of the
 * branch the forward code's own comparison selects (gap = d - nhat . x_p > 0, and
 * k phi (1 + c phid) > 0): a point that does not push (f_n = 0) contributes exactly zero, also at
 * a kink, where the function has one-sided derivatives only.  Friction (mu > 0) is differentiated
 * through its regularisation; mu == 0 folds those terms away.  The contact terms are evaluated in
 * reverse mode (contact_vjp_body.hip.hpp): O(n + P) work per step beside the column sweeps.
 *
 * Checks, in order: as multibody_rollout_vjp_batch_* (handle, batch >= 0, ld >= batch, batch == 0
 * RB_OK, K < 0 / K == 0 RB_ERR_ARG, a NULL array RB_ERR_NULL, an aliased output or workspace
 * RB_ERR_ARG), then a handle without a contact set RB_ERR_UNSUPPORTED (rb_last_error() names
 * multibody_with_contacts), then the scope.  Batches are split at 2^28 per launch.
 *
 * Scope: multibody_rollout_vjp_*'s -- serial revolute chains (z-axis or RB_MODEL_GENERAL_AXES) up to
 * 12 links; kinematic trees, prismatic joints, a floating base and longer chains return
 * RB_ERR_UNSUPPORTED and rb_last_error() names the condition, as does hipRTC disabled or failed
 * (with the log).  SoA rows only.
 *
 * Relation to multibody_rollout_contact_batch_*: the trajectory differentiated is the contact
 * rollout of the mass-matrix forward dynamics.  For chains of 9 to 12 links
 * multibody_rollout_contact_batch_* integrates the articulated-body form instead, so the two
 * trajectories agree to rounding, not bit for bit.
 *
 * Input domain: q_k, v_k, tau_k and the contact wrench are checked at every step, all of them before
 * the first store; a configuration that leaves the domain at any step gets NaN in every element of
 * g_q0, g_qd0 and g_tau, the others are unaffected.  The cotangents are NOT checked.
 *
 * Accuracy (tests/test_contact_vjp_host.py, tests/test_gpu_contact_vjp.py; reference
 * tests/contact_vjp_ref.py: Richardson central differences, h = 2e-3, of a rollout assembled from the
 * reference contact law and the fp64 oracle's forward dynamics, along a unit direction, dt = 1e-3,
 * K = 3, about 40% of the points pushing): fp64 |<g, d> - ref| <= 1e-7 (1 + |ref|) wherever that
 * reference is self-consistent to 1e-8 (a configuration that crosses a kink within the step is not);
 * measured on the MI355X (B = 257, first 40 configurations, 37-38 qualify): 4.4e-10 FR3, 4.7e-10 on 12
 * links, 1.3e-10 on the general-axis 7-link chain, and 4.4e-10 against differences of
 * multibody_rollout_contact_batch_f64 itself (FR3).  The kernel agrees with the host form of the same
 * lane body to 7.02e-13 relative (measured 7.01e-14, K = 3), a configuration with a point exactly on
 * the plane aside (its branch is decided by the last bit).  fp32 against the fp64 kernel on the same
 * fp32-rounded inputs, per output array and configuration, configurations within 1e-3 m of the plane or
 * with |1 + c phid| < 1e-2 while penetrating aside (a rounding flip of the branch there is not an
 * error; 2% of FR3's): max|d| <= 6e-4 (1 + max|ref|) -- 4x the measured maximum, 1.47e-4 (12 links;
 * FR3 2.0e-5). */
int multibody_rollout_contact_vjp_batch_f32(const Multibody *mb, const float *q, const float *qd,
                                            const float *tau_seq, double dt, int K, const float *gq,
                                            const float *gqd, float *g_q0, float *g_qd0, float *g_tau, float *work,
                                            int64_t batch, int64_t ld, void *stream);
int multibody_rollout_contact_vjp_batch_f64(const Multibody *mb, const double *q, const double *qd,
                                            const double *tau_seq, double dt, int K, const double *gq,
                                            const double *gqd, double *g_q0, double *g_qd0, double *g_tau,
                                            double *work, int64_t batch, int64_t ld, void *stream);
/* Blocking host-pointer forms: contiguous host arrays (ld = batch); the workspace is internal. */
int multibody_rollout_contact_vjp_batch_host_f32(const Multibody *mb, const float *q, const float *qd,
                                                 const float *tau_seq, double dt, int K, const float *gq,
                                                 const float *gqd, float *g_q0, float *g_qd0, float *g_tau,
                                                 int64_t batch);
int multibody_rollout_contact_vjp_batch_host_f64(const Multibody *mb, const double *q, const double *qd,
                                                 const double *tau_seq, double dt, int K, const double *gq,
                                                 const double *gqd, double *g_q0, double *g_qd0, double *g_tau,
                                                 int64_t batch);
/* One configuration, fp64, [K][n] arrays, on the calling thread: the same lane body compiled for
 * the host, no GPU involved (an FMA3 / AVX2 CPU, else RB_ERR_UNSUPPORTED). */
int multibody_rollout_contact_vjp(const Multibody *mb, const double *q, const double *qd, const double *tau_seq,
                                  double dt, int K, const double *gq, const double *gqd, double *g_q0,
                                  double *g_qd0, double *g_tau);
/* Inspection of that kernel (no kind number), as multibody_contact_jit_source / _compile: a model
 * out of scope or without a contact set has the empty source / -RB_ERR_UNSUPPORTED. */
int multibody_contact_vjp_jit_source(const Multibody *mb, int f64, int64_t batch, char *buf, int64_t cap);
int64_t multibody_contact_vjp_jit_compile(const Multibody *mb, int f64, int64_t batch, const char *arch);

/* ---- reverse-mode gradient of the inverse dynamics --------------------------------- */
/* The gradient of a scalar cost of tau = rnea_ext(q, qd, qdd, fext) with respect to all four inputs,
 * for every model multibody_rnea_ext_* runs on -- the first derivative in this ABI that works on
 * kinematic trees, prismatic joints and a floating base.  One O(n) reverse sweep of the RNEA: it
 * reads 4 n + 6 n rows and writes 3 n + 6 n, where multibody_rnea_deriv_* writes 2 n^2.
 *
 * Definition, for one configuration and the cotangent w [n] of tau:
 *   L      = sum_i w_i tau_i
 *   g_q    [n]     g_q[k]   = sum_i w_i d tau_i / d q_k
 *   g_qd   [n]     g_qd[k]  = sum_i w_i d tau_i / d qd_k
 *   g_qdd  [n]     = sym(H(q)) w           (the RNEA is affine in qdd with slope H, multibody_crba's)
 *   g_fext [6 n]   g_fext_j = -J_j(q) w    (rows [lin; rot], link j's URDF link frame: minus what
 *                                           multibody_link_vel(q, w) returns for link j)
 * Frames, row orders and the gravity convention are those of multibody_rnea_ext_* and
 * multibody_link_vel_*.  No Jacobian matrix is formed or stored.
 *
 * Layout: SoA rows of leading dimension ld; q, qd, qdd, w, g_q, g_qd, g_qdd [n][ld]; fext, g_fext
 * [6 n][ld] as multibody_rnea_ext takes fext.
 *
 * Two families, every array required in both (the contract of every batched entry point here):
 *   multibody_rnea_vjp_batch_*        tau = rnea_ext(q, qd, qdd, fext); also returns g_fext
 *   multibody_rnea_vjp_plain_batch_*  tau = rnea(q, qd, qdd): a kernel variant that has no wrench rows
 * The single-configuration multibody_rnea_vjp serves both: fext == NULL selects the plain RNEA (g_fext
 * must then be NULL too, else RB_ERR_ARG), and with fext given g_fext may still be NULL (not evaluated).
 *
 * Checks, in order: handle (RB_ERR_NULL), batch >= 0, ld >= batch (RB_ERR_ARG), batch == 0 (RB_OK,
 * nothing else looked at), a NULL array (RB_ERR_NULL), the single form's g_fext without fext
 * (RB_ERR_ARG), an output that is also an input or is passed twice (RB_ERR_ARG), then hipRTC.
 *
 * Scope: every model the external-wrench kernels run -- serial chains under either reading and of
 * every supported length, general axes, kinematic trees, prismatic joints, a floating base.
 * Model-specialised (hipRTC) kernels only, no kind number: with hipRTC disabled or failed
 * RB_ERR_UNSUPPORTED with the log.  One configuration per lane, SoA rows only, batches split at 2^28.
 * The single-configuration form has the scope of multibody_rnea_ext.
 *
 * Input domain: q, qd, qdd and fext are checked as in multibody_rnea_ext_*: a configuration with a
 * NaN / Inf input or an angle past the bound gets NaN in every element of every output, the others
 * are unaffected; every input is checked before the configuration's first store.  The cotangent w is
 * NOT checked (a NaN there propagates by arithmetic), as gq / gqd of multibody_rollout_vjp_*.
 *
 * Algorithm (rnea_vjp_body.hip.hpp), in spatial notation (X_j parent -> child, x / x* the motion /
 * force cross products, e_j the wrench).  Pass A, root to leaf, is the RNEA's forward sweep fused
 * with phi_j = X_j phi_p + S_j w_j (phi_base = 0), the adjoint of the transmitted force: L = sum_j
 * phi_j . f_j and g_fext_j = -phi_j.  Pass B, leaf to root, accumulates F_j (the RNEA's), A_j = I_j
 * phi_j + children and V_j = -phi_j x* (I_j v_j) - I_j (v_j x phi_j) + qd_j (S_j x* A_j) + children,
 * each handed up as X_j^T . , and reads off g_qdd_j = S_j . A_j, g_qd_j = S_j . V_j + A_j . (v_j x S_j),
 * g_q_j = phi_j . (S_j x* F_j) - A_j . (S_j x X_j a_p) - V_j . (S_j x v_j).  Every output leaves in
 * pass B, after the last wrench row has been checked.
 *
 * Accuracy (tests/test_rnea_vjp_host.py, tests/test_gpu_rnea_vjp.py; reference tests/rnea_vjp_ref.py:
 * Richardson central differences, h = 1e-3, of w . (oracle rnea - J^T fext) along a direction scaled to
 * the inputs' ranges).  fp64: |<g, d> - ref| <= 1e-7 (1 + |ref|) wherever the reference is
 * self-consistent to 1e-8; g_qdd = sym(H) w with H of multibody_crba and g_fext = -link_vel(q, w) to
 * 1e-9 scaled; g_q, g_qd against multibody_rnea_deriv contracted with w to 1e-8 scaled (serial
 * chains).  The kernel agrees with the host form of the same lane body to 2.52e-14 relative (10x the
 * measured 2.52e-15).  fp32 against the fp64 kernel on the same fp32-rounded inputs, per configuration
 * and output array: max|d| <= 2e-5 (1 + max|ref|) -- 7x the measured maximum, 2.71e-6 (floating base).
 * Measured (MI355X, B = 257, first 40 configurations differenced, all 40 qualify): fp64 against the
 * reference 4.7e-11 FR3 / 4.9e-11 12 links with general axes / 3.6e-10 16 links / 1.2e-11 the 9-joint
 * tree / 1.1e-10 floating base (the reference's own self-consistency is 1.2e-9 at most); g_qdd against
 * crba 9.6e-16 at most, g_fext against link_vel bit for bit, g_q / g_qd against rnea_deriv 7.8e-16 at
 * most; the plain kernel against the wrench kernel at fext = 0 bit for bit; fp32 8.4e-7 FR3 / 7.8e-7 the
 * tree / 2.7e-6 floating base.  Single-configuration form on the host: 7.0e-11 at most against the
 * reference (12 links), identities 1.6e-15 at most (30 links).
 * Timing (tools/rnea_vjp_bench.py, MI355X, 2^20 configurations, HIP-graph replay, interleaved with its
 * neighbours): FR3 fp64 wrench form 253.0 us (0.55 of HBM peak), plain 107.3 (0.48), beside rnea_ext 115.4
 * and rnea_deriv plus the two products with w in torch 770.0; fp32 97.8 (0.71) / 42.2 (0.61) beside 52.3 and
 * 394.9; floating base fp64 789.1 (0.35) / 296.7 (0.35) beside rnea_ext 543.8, fp32 271.1 / 102.1 beside
 * 104.9.  FR3 uses no scratch; the floating base's fp64 wrench kernel spills. */
int multibody_rnea_vjp_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                 const float *fext, const float *w, float *g_q, float *g_qd, float *g_qdd,
                                 float *g_fext, int64_t batch, int64_t ld, void *stream);
int multibody_rnea_vjp_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                 const double *fext, const double *w, double *g_q, double *g_qd, double *g_qdd,
                                 double *g_fext, int64_t batch, int64_t ld, void *stream);
int multibody_rnea_vjp_plain_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                       const float *w, float *g_q, float *g_qd, float *g_qdd, int64_t batch,
                                       int64_t ld, void *stream);
int multibody_rnea_vjp_plain_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                       const double *w, double *g_q, double *g_qd, double *g_qdd, int64_t batch,
                                       int64_t ld, void *stream);
/* Blocking host-pointer forms: contiguous host arrays (ld = batch). */
int multibody_rnea_vjp_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                      const float *fext, const float *w, float *g_q, float *g_qd, float *g_qdd,
                                      float *g_fext, int64_t batch);
int multibody_rnea_vjp_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                      const double *fext, const double *w, double *g_q, double *g_qd, double *g_qdd,
                                      double *g_fext, int64_t batch);
int multibody_rnea_vjp_plain_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                            const float *w, float *g_q, float *g_qd, float *g_qdd, int64_t batch);
int multibody_rnea_vjp_plain_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                            const double *w, double *g_q, double *g_qd, double *g_qdd, int64_t batch);
/* One configuration, fp64, caller-provided outputs, on the calling thread: the same lane body compiled
 * for the host, no GPU needed.  fext and g_fext may be NULL as described above. */
int multibody_rnea_vjp(const Multibody *mb, const double *q, const double *qd, const double *qdd, const double *fext,
                       const double *w, double *g_q, double *g_qd, double *g_qdd, double *g_fext);
/* Inspection of those kernels (no kind number): ext != 0 selects the wrench form, else the plain one;
 * otherwise as multibody_ext_jit_source / _compile. */
int multibody_rnea_vjp_jit_source(const Multibody *mb, int ext, int f64, int64_t batch, char *buf, int64_t cap);
int64_t multibody_rnea_vjp_jit_compile(const Multibody *mb, int ext, int f64, int64_t batch, const char *arch);

/* ---- reverse-mode gradient of the forward dynamics --------------------------------- */
/* The gradient of a scalar cost of qdd = fd_ext(q, qd, tau, fext) with respect to all four inputs, for
 * every model multibody_fd_ext_* runs on (multibody_fd_deriv_* stops at serial revolute chains of up to
 * 12 links), from one launch that also returns qdd.  It reads 4 n + 6 n rows and writes 4 n + 6 n; no
 * mass matrix leaves the kernel.
 *
 * Definition, for one configuration and the cotangent w [n] of qdd:
 *   L      = sum_i w_i qdd_i
 *   qdd    [n]     what multibody_fd_ext_batch_* returns for the same inputs, bit for bit
 *   g_tau  [n]     = mu = sym(H(q))^-1 w   (H of multibody_crba)
 *   g_q    [n]     = -(g_q  of multibody_rnea_vjp at (q, qd, qdd, fext) with the cotangent mu)
 *   g_qd   [n]     = -(g_qd of the same)
 *   g_fext [6 n]   g_fext_j = +J_j(q) mu   (rows [lin; rot], link j's URDF link frame: what
 *                                           multibody_link_vel(q, mu) returns for link j)
 * which follows from H dqdd + d rnea_ext(q, qd, qdd, fext) = dtau.  Frames, row orders and the gravity
 * convention are those of multibody_fd_ext_* and multibody_rnea_vjp_*.
 *
 * Layout: SoA rows of leading dimension ld; q, qd, tau, w, qdd, g_q, g_qd, g_tau [n][ld]; fext, g_fext
 * [6 n][ld] as multibody_fd_ext takes fext.
 *
 * Two families, every array required in both (the contract of every batched entry point here):
 *   multibody_fd_vjp_batch_*        qdd = fd_ext(q, qd, tau, fext); also returns g_fext
 *   multibody_fd_vjp_plain_batch_*  qdd = fd_ext(q, qd, tau, 0): a kernel variant that has no wrench rows
 *                                   (the wrench family's results at fext = 0, bit for bit)
 * The single-configuration multibody_fd_vjp serves both: fext == NULL selects the plain form (g_fext must
 * then be NULL too, else RB_ERR_ARG), and with fext given g_fext may still be NULL (not evaluated).
 *
 * Checks, in order: handle (RB_ERR_NULL), batch >= 0, ld >= batch (RB_ERR_ARG), batch == 0 (RB_OK,
 * nothing else looked at), a NULL array (RB_ERR_NULL), the single form's g_fext without fext
 * (RB_ERR_ARG), an output that is also an input or is passed twice (RB_ERR_ARG), then hipRTC.
 *
 * Scope: every model multibody_fd_ext_batch_* runs -- serial chains under either reading and of every
 * supported length, general axes, kinematic trees, prismatic joints, a floating base.
 * Model-specialised (hipRTC) kernels only, no kind number: with hipRTC disabled or failed
 * RB_ERR_UNSUPPORTED with the log.  One configuration per lane, SoA rows only, batches split at 2^28.
 * The single-configuration form has the scope of multibody_rnea_vjp.
 *
 * Input domain: q, qd, tau and fext are checked as in multibody_fd_ext_*: a configuration with a NaN /
 * Inf input or an angle past the bound gets NaN in every element of every output, the others are
 * unaffected; every input is checked before the configuration's first store.  The cotangent w is NOT
 * checked (a NaN there propagates by arithmetic).
 *
 * Algorithm (fd_vjp_body.hip.hpp), two stages per lane.  Stage 1 is the forward dynamics in the form
 * multibody_fd_ext takes for the model, with a second right-hand side: the mass-matrix form (serial
 * chains up to 12 links) factorises H once and solves L D L^T x = b for (tau - C) and for w; the
 * articulated-body form (longer chains, trees, a floating base) carries a second bias force and a
 * second u / D through its passes 2 and 3 on the same articulated inertias.  Stage 2 is the reverse
 * sweep of multibody_rnea_vjp at (q, qd, qdd; mu), its outputs negated.  The wrench rows are fetched by
 * the link step that consumes them in each stage: they are read twice and never held together.
 *
 * Accuracy (tests/test_fd_vjp_host.py, tests/test_gpu_fd_vjp.py; reference tests/fd_vjp_ref.py: Richardson
 * central differences, h = 1e-3, of w . (oracle fd at tau + J^T fext) along a direction scaled to the
 * inputs' ranges).  fp64: |<g, d> - ref| <= 1e-7 (1 + |ref|) wherever the reference is self-consistent
 * to 1e-8; qdd = multibody_fd_ext, sym(H) g_tau = w with H of multibody_crba and g_fext = link_vel(q,
 * g_tau) to 1e-9 scaled; g_q, g_qd, g_tau against multibody_fd_deriv contracted with w to 1e-8 scaled
 * (serial chains up to 12 links).  Measured (MI355X, B = 257, first 40 configurations differenced):
 * against the reference 8.1e-10 FR3 / 6.5e-10 12 links with general axes / 3.1e-9 16 links (39 of 40
 * qualify) / 3.0e-11 the 9-joint tree / 2.0e-11 floating base; qdd against multibody_fd_ext_batch bit for
 * bit; sym(H) g_tau against w 4.4e-13 at most (16 links); g_fext against link_vel bit for bit; the plain
 * kernel against the wrench kernel at fext = 0 bit for bit.  Against -multibody_rnea_vjp_batch at (q, qd,
 * qdd, g_tau, fext): g_qd and g_fext bit for bit, g_q within 2.86e-15 scaled (10x the measured 2.86e-16:
 * that kernel forms the link forces about the link origin, this one about the centre of mass, as
 * multibody_fd_ext does).  The kernel agrees with the host form of the same lane body to 2.53e-13
 * (10x the measured 2.53e-14).  fp32 against the fp64 kernel on the same fp32-rounded inputs, per
 * configuration and output array: max|d| <= 1.6e-4 (1 + max|ref|) -- about 7x the measured maximum,
 * 2.22e-5 (FR3; the tree 1.8e-6, floating base 5.5e-6).  Single-configuration form on the host: 4.3e-9 at
 * most against the reference (30 links, 19 of 20 qualify), identities 2.7e-12 at most (30 links),
 * multibody_fd_deriv 5.0e-14 at most.
 * Timing (tools/fd_vjp_bench.py, profiles/fd_vjp/fd_vjp_bench.json; MI355X, 2^20 configurations, HIP-graph
 * replay, interleaved with its neighbours, median us): FR3 fp64 wrench form 378.2 (0.39 of HBM peak), plain
 * 159.3 (0.37), beside fd_ext 110.9, rnea_vjp 261.2 and the unfused composition (fd_ext, crba, a batched solve
 * in torch, rnea_vjp; timed eagerly) 4909.9; fp32 126.9 (0.58) / 72.5 (0.40) beside 53.1, 99.5 and 3632.7;
 * floating base fp64 1707.7 (0.17) / 627.1 (0.19) beside fd_ext 522.3 and rnea_vjp 798.8, fp32 696.1 / 326.3
 * beside 125.8 and 268.6.  So on FR3 one launch costs what fd_ext plus rnea_vjp cost and is 13x / 29x faster
 * than the composition; on the floating base it is slower than those two launches together (one wave per
 * SIMD at 494-512 registers).  Resources (profiles/fd_vjp/resources.json): FR3 and the tree use
 * no scratch; every variant of the 30-link chain and the fp64 variants of the floating base spill. */
int multibody_fd_vjp_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *tau,
                               const float *fext, const float *w, float *qdd, float *g_q, float *g_qd, float *g_tau,
                               float *g_fext, int64_t batch, int64_t ld, void *stream);
int multibody_fd_vjp_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                               const double *fext, const double *w, double *qdd, double *g_q, double *g_qd,
                               double *g_tau, double *g_fext, int64_t batch, int64_t ld, void *stream);
int multibody_fd_vjp_plain_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *tau,
                                     const float *w, float *qdd, float *g_q, float *g_qd, float *g_tau, int64_t batch,
                                     int64_t ld, void *stream);
int multibody_fd_vjp_plain_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                                     const double *w, double *qdd, double *g_q, double *g_qd, double *g_tau,
                                     int64_t batch, int64_t ld, void *stream);
/* Blocking host-pointer forms: contiguous host arrays (ld = batch). */
int multibody_fd_vjp_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *tau,
                                    const float *fext, const float *w, float *qdd, float *g_q, float *g_qd,
                                    float *g_tau, float *g_fext, int64_t batch);
int multibody_fd_vjp_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                                    const double *fext, const double *w, double *qdd, double *g_q, double *g_qd,
                                    double *g_tau, double *g_fext, int64_t batch);
int multibody_fd_vjp_plain_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *tau,
                                          const float *w, float *qdd, float *g_q, float *g_qd, float *g_tau,
                                          int64_t batch);
int multibody_fd_vjp_plain_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                                          const double *w, double *qdd, double *g_q, double *g_qd, double *g_tau,
                                          int64_t batch);
/* One configuration, fp64, caller-provided outputs, on the calling thread: the same lane body compiled
 * for the host, no GPU needed.  fext and g_fext may be NULL as described above. */
int multibody_fd_vjp(const Multibody *mb, const double *q, const double *qd, const double *tau, const double *fext,
                     const double *w, double *qdd, double *g_q, double *g_qd, double *g_tau, double *g_fext);
/* Inspection of those kernels (no kind number): ext != 0 selects the wrench form, else the plain one;
 * otherwise as multibody_ext_jit_source / _compile. */
int multibody_fd_vjp_jit_source(const Multibody *mb, int ext, int f64, int64_t batch, char *buf, int64_t cap);
int64_t multibody_fd_vjp_jit_compile(const Multibody *mb, int ext, int f64, int64_t batch, const char *arch);

/* ---- batched host-pointer entry points (blocking) ------------------------------ */
int multibody_rnea_batch_host_f64(const Multibody *mb, const double *q, const double *qd,
                                  const double *qdd, double *tau, int64_t batch);
int multibody_fd_batch_host_f64(const Multibody *mb, const double *q, const double *qd,
                                const double *tau, double *qdd, int64_t batch);
int multibody_rnea_batch_host_f32(const Multibody *mb, const float *q, const float *qd,
                                  const float *qdd, float *tau, int64_t batch);
int multibody_fd_batch_host_f32(const Multibody *mb, const float *q, const float *qd,
                                const float *tau, float *qdd, int64_t batch);

/* ---- synthetic inputs, generated on device ------------------------------------- */
/* x[j*ld + b] = lo[j] + (hi[j]-lo[j]) * u(seed, j, b), u = splitmix64 -> [0,1) with
 * 53-bit (f64) / 24-bit (f32) mantissa; lo/hi are host arrays of n_rows. */
int rb_fill_uniform_f32(float *x, int n_rows, int64_t batch, int64_t ld, const double *lo,
                        const double *hi, uint64_t seed, void *stream);
int rb_fill_uniform_f64(double *x, int n_rows, int64_t batch, int64_t ld, const double *lo,
                        const double *hi, uint64_t seed, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RIGIDBODY_BATCH_H */
