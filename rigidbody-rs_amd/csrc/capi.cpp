// capi.cpp -- the extern "C" boundary (include/rigidbody.h, include/rigidbody_batch.h).
//
// Drop-in for the Rust cdylib rigidbody_bindings (rigidbody_bindings/src/lib.rs:8-78):
// same six symbols and result layouts, plus batched device-pointer entry points.
// Every batched entry point runs a HIP kernel on the current device (no CPU fallback).  The
// reference's single-configuration queries run on the calling host thread with the same
// lane bodies compiled for the host (host_eval.cpp: SURVEY §8(d) config 1 is a CPU path, and
// a GPU round trip costs ~25x the recursion), unless the model needs hipRTC (trees) or the
// caller asks for the GPU (tuning single_gpu).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <initializer_list>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rigidbody_batch.h"
#include "kernels.hpp"
#include "model.hpp"
#include "tuning.hpp"
#include "jit.hpp"
#include "device_cache.hpp"
#include "host_eval.hpp"

#include "fr3_embedded.inc"  // kFr3Urdf: compact FR3 description (tools/gen_fixtures.py)

#define RB_VERSION "rigidbody-rs_amd 0.2.0 (gfx950)"

static const char *const kKindMsg = "kind must be 0 rnea, 1 fd, 2 crba, 3 rollout, 4 fwd_kin, 5 jac, 6 rnea_fd, 7 rnea_deriv or 8 fd_deriv";

namespace {

thread_local std::string g_last_error;
// Why a launcher refused (a tree model without its hipRTC kernel); hip_err reports it.
thread_local std::string t_launch_note;

int set_err(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

int hip_err(hipError_t e, const char *where) {
    std::string msg = std::string(where) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")";
    if (!t_launch_note.empty()) {
        msg += ": " + t_launch_note;
        t_launch_note.clear();
        return set_err(RB_ERR_UNSUPPORTED, msg);
    }
    return set_err(RB_ERR_HIP, msg);
}

bool env_flag(const char *name, bool dflt) {
    const char *v = std::getenv(name);
    if (!v || !*v) return dflt;
    return !(v[0] == '0' || v[0] == 'n' || v[0] == 'N' || v[0] == 'f' || v[0] == 'F');
}

// fp32 kernels use the hardware sin/cos (v_sin_f32 / v_cos_f32) unless RB_FAST_TRIG=0.
bool fast_trig() {
    static const bool fast = env_flag("RB_FAST_TRIG", true);
    return fast;
}

}  // namespace

struct Multibody {
    rbamd::Model model;
    std::vector<float> pk32;
    std::vector<double> pk64;
    std::vector<double> ra64;  // every link's axis frame (Model::axis_frames): the host external-wrench forms
    mutable rbamd::DeviceCache cache;  // constants and hipRTC kernels on the devices it has run on
};

namespace {

constexpr int kMaxTreeDof = 64;

Multibody *make(rbamd::Model &&m) {
    if (!m.axes_supported()) {
        set_err(RB_ERR_UNSUPPORTED,
                "non-z joint axis: the reference injects joint motion about local z "
                "(multibody.rs:130-138,144); pass RB_MODEL_GENERAL_AXES for general axes");
        return nullptr;
    }
    // The reference's serial revolute chains run on the precompiled kernels (dofs.hpp) or
    // their model-specialised versions; trees and prismatic joints only on the latter, which
    // exist for any DOF count.
    if (m.serial_revolute() ? !rbamd::dof_supported(m.n) : m.n > kMaxTreeDof) {
        set_err(RB_ERR_DOF, m.serial_revolute() ? "no kernel compiled for " + std::to_string(m.n) + " DOF"
                                                : "tree models support at most 64 DOF, got " + std::to_string(m.n));
        return nullptr;
    }
    Multibody *mb = new Multibody();
    mb->pk32 = m.pack_f32();
    mb->pk64 = m.pack_f64();
    mb->ra64 = m.axis_frames();
    mb->model = std::move(m);
    return mb;
}

// Device copy of the packed model constants on the current device (uploaded once).
template <typename T>
int device_consts(const Multibody *mb, const T **out) {
    const char *where = nullptr;
    hipError_t e;
    if constexpr (sizeof(T) == 4) e = mb->cache.consts(mb->pk32, out, &where);
    else e = mb->cache.consts(mb->pk64, out, &where);
    return e == hipSuccess ? RB_OK : hip_err(e, where);
}

// A tree / prismatic model has no precompiled kernel: without its hipRTC kernel the launch
// is refused (hipErrorNotSupported, reported as RB_ERR_UNSUPPORTED with the reason).
hipError_t no_generic(const Multibody *mb, const char *what = "kinematic-tree / prismatic models run") {
    std::string why = std::string(what) + " only on model-specialised (hipRTC) kernels";
    if (!rbamd::jit_enabled()) {
        why += ", which are disabled (RB_JIT=0 / rb_set_tuning(\"jit\", 0))";
    } else {
        for (const std::string &err : mb->cache.jit_errors()) why += "; hipRTC: " + err.substr(0, 400);
    }
    t_launch_note = why;
    return hipErrorNotSupported;
}

// Serial revolute chains take the precompiled kinematics kernels only when the (experimental)
// tuning `kin_jit` is 0.
bool kin_precompiled(const Multibody *mb) {
    return mb->model.serial_revolute() && rbamd::tuning().kin_jit == 0;
}

// The hipRTC kernel a launch of B configurations of `kind` takes, or nullptr for the generic
// path.  The launchers and the inspection entry points (multibody_kernel_path_ex / _form_ex)
// resolve through this one; which variant it is, is jit_resolve's business (jit.cpp), CRBA's
// always-precise trig included.
const rbamd::JitKernel *kernel_for(const Multibody *mb, rbamd::JitKind kind, bool f64, uint32_t B, bool tiled) {
    // fwd_kin / jac: the hipRTC kernels (tree_body.hip.hpp fwd_kin_tree / jac_tree, the model's
    // topology and constants compiled in) for every model; serial revolute chains fall back to the
    // precompiled kernels (kinematics.hip) when hipRTC is off or failed.  FR3 2^20: fwd_kin fp64
    // 18.2 vs 26.4 us precompiled, fp32 9.6 vs 11.3; the Jacobian is store-bound, equal (89.2 vs
    // 89.5 / 41.4 vs 41.3 us; profiles/r04/ab/ab_fk*.log, ab_jac*.log).
    if ((kind == rbamd::JitKind::FwdKin || kind == rbamd::JitKind::Jac) && kin_precompiled(mb)) return nullptr;
    // the fused inverse + forward dynamics exists for serial chains on the mass-matrix form only
    // (jit_fd_form is 1 for this kind on every model that is not a serial revolute chain)
    if (kind == rbamd::JitKind::RneaFd && rbamd::jit_fd_form(mb->model, rbamd::JitKind::RneaFd) != 2) return nullptr;
    return mb->cache.kernel(mb->model, rbamd::jit_resolve(mb->model, kind, f64, B, tiled, fast_trig()));
}

hipError_t jit_launch(const rbamd::JitKernel *jk, uint32_t B, void **args, hipStream_t s) {
    return hipModuleLaunchKernel(jk->function, rbamd::jit_grid(*jk, B), 1, 1, jk->block, 1, 1, 0, s, args, nullptr);
}

// Strides (elements) the JIT lane kernels take for arrays of rows_in / rows_out rows per
// configuration: the row stride, and the stride from one 256-configuration block to the next --
// 256 for SoA rows of length ld, rows * 256 for the tiled layout (kernels.hpp).
struct TileStrides {
    int64_t lda, bs_in, bs_out;
};
TileStrides tile_strides(bool tiled, int64_t ld, int64_t rows_in, int64_t rows_out) {
    if (!tiled) return {ld, 256, 256};
    return {256, rows_in * 256, rows_out * 256};
}

// One launch of B configurations of `kind`: the model-specialised kernel with `args` (pointers
// to the caller's locals, in the kernel's parameter order) where kernel_for has one, else
// `fallback()` -- the precompiled launcher, no_generic, or another launcher.
template <size_t N, typename Fallback>
hipError_t launch_any(const Multibody *mb, rbamd::JitKind kind, bool f64, uint32_t B, bool tiled, hipStream_t s,
                      void *(&args)[N], Fallback fallback) {
    if (B == 0) return hipSuccess;
    if (const rbamd::JitKernel *jk = kernel_for(mb, kind, f64, B, tiled)) return jit_launch(jk, B, args, s);
    return fallback();
}

// tiled: the [ceil(B/256)][n][256] layout (kernels.hpp); the JIT lane kernels and the
// generic lane kernels take it through their block stride (the generic grid-stride RNEA is
// SoA-only and never chosen for it).
template <typename T>
hipError_t launch_rnea_any(const Multibody *mb, const T *mdl, const T *q, const T *qd, const T *qdd, T *tau,
                           uint32_t B, int64_t ld, hipStream_t s, bool tiled = false) {
    const int n = mb->model.n;
    TileStrides st = tile_strides(tiled, ld, n, n);
    void *args[] = {&q, &qd, &qdd, &tau, &B, &st.lda, &st.bs_in};
    return launch_any(mb, rbamd::JitKind::Rnea, sizeof(T) == 8, B, tiled, s, args, [&] {
        if (!mb->model.serial_revolute()) return no_generic(mb);
        return rbamd::launch_rnea<T>(n, mdl, q, qd, qdd, tau, B, ld, s, fast_trig(), tiled);
    });
}

template <typename T>
hipError_t launch_fd_any(const Multibody *mb, const T *mdl, const T *q, const T *qd, const T *tau, T *qdd,
                         uint32_t B, int64_t ld, hipStream_t s, bool tiled = false) {
    const int n = mb->model.n;
    TileStrides st = tile_strides(tiled, ld, n, n);
    void *args[] = {&q, &qd, &tau, &qdd, &B, &st.lda, &st.bs_in};
    return launch_any(mb, rbamd::JitKind::Fd, sizeof(T) == 8, B, tiled, s, args, [&] {
        if (!mb->model.serial_revolute()) return no_generic(mb);
        return rbamd::launch_aba<T>(n, mdl, q, qd, tau, qdd, B, ld, s, fast_trig(), tiled);
    });
}

// Inverse + forward dynamics of the same (q, qd) (config 4's pair): one fused hipRTC launch
// (fdh_body.hip.hpp idfd_lane) for models on the mass-matrix forward dynamics; otherwise -- the
// ABA models (trees, chains over 12 links), hipRTC off or failed -- the RNEA launch then the
// forward-dynamics launch, the same results.
template <typename T>
hipError_t launch_idfd_any(const Multibody *mb, const T *mdl, const T *q, const T *qd, const T *qdd, const T *tau_in,
                           T *tau, T *qdd_out, uint32_t B, int64_t ld, hipStream_t s, bool tiled = false) {
    TileStrides st = tile_strides(tiled, ld, mb->model.n, mb->model.n);
    void *args[] = {&q, &qd, &qdd, &tau_in, &tau, &qdd_out, &B, &st.lda, &st.bs_in};
    return launch_any(mb, rbamd::JitKind::RneaFd, sizeof(T) == 8, B, tiled, s, args, [&] {
        hipError_t e = launch_rnea_any<T>(mb, mdl, q, qd, qdd, tau, B, ld, s, tiled);
        if (e != hipSuccess) return e;
        return launch_fd_any<T>(mb, mdl, q, qd, tau_in, qdd_out, B, ld, s, tiled);
    });
}

template <typename T>
hipError_t launch_rollout_any(const Multibody *mb, const T *mdl, T *q, T *qd, const T *tau_seq, T dt, int K, T *traj,
                              uint32_t B, int64_t ld, hipStream_t s) {
    void *args[] = {&q, &qd, &tau_seq, &dt, &K, &traj, &B, &ld};
    return launch_any(mb, rbamd::JitKind::Rollout, sizeof(T) == 8, B, false, s, args, [&] {
        if (!mb->model.serial_revolute()) return no_generic(mb);
        return rbamd::launch_rollout<T>(mb->model.n, mdl, q, qd, tau_seq, dt, K, traj, B, ld, s, fast_trig());
    });
}

template <typename T>
hipError_t launch_crba_any(const Multibody *mb, const T *mdl, const T *q, T *H, uint32_t B, int64_t ld,
                           hipStream_t s, bool tiled = false) {
    const int64_t n = mb->model.n;
    TileStrides st = tile_strides(tiled, ld, n, n * n);
    void *args[] = {&q, &H, &B, &st.lda, &st.bs_in, &st.bs_out};
    return launch_any(mb, rbamd::JitKind::Crba, sizeof(T) == 8, B, tiled, s, args, [&] {
        if (!mb->model.serial_revolute()) return no_generic(mb);
        return rbamd::launch_crba<T>(mb->model.n, mdl, q, H, B, ld, s, tiled);
    });
}

template <typename T>
hipError_t launch_kin_any(const Multibody *mb, bool jac, const T *mdl, const T *q, T *out, uint32_t B, int64_t ld,
                          hipStream_t s, bool tiled = false) {
    const int64_t n = mb->model.n;
    TileStrides st = tile_strides(tiled, ld, n, jac ? 6 * n : 3);
    void *args[] = {&q, &out, &B, &st.lda, &st.bs_in, &st.bs_out};
    return launch_any(mb, jac ? rbamd::JitKind::Jac : rbamd::JitKind::FwdKin, sizeof(T) == 8, B, tiled, s, args, [&] {
        if (!mb->model.serial_revolute()) return no_generic(mb);
        const bool fast = sizeof(T) == 4 && fast_trig();
        return jac ? rbamd::launch_jac<T>(mb->model.n, mdl, q, out, B, ld, s, fast, tiled)
                   : rbamd::launch_fwd_kin<T>(mb->model.n, mdl, q, out, B, ld, s, fast, tiled);
    });
}

// Analytical derivatives (rnea_deriv_body.hip.hpp): model-specialised kernels only, SoA rows; a
// NULL output is neither evaluated nor stored.  Without the kernel (hipRTC off or failed) the
// launch is refused as a tree model's is.
template <typename T>
hipError_t launch_rnea_deriv(const Multibody *mb, const T *q, const T *qd, const T *qdd, T *dq, T *dqd, uint32_t B,
                             int64_t ld, hipStream_t s) {
    int64_t bs = 256;
    void *args[] = {&q, &qd, &qdd, &dq, &dqd, &B, &ld, &bs};
    return launch_any(mb, rbamd::JitKind::RneaDeriv, sizeof(T) == 8, B, false, s, args,
                      [&] { return no_generic(mb, "the dynamics derivatives run"); });
}

template <typename T>
hipError_t launch_fd_deriv(const Multibody *mb, const T *q, const T *qd, const T *tau, T *qdd, T *dq, T *dqd, T *dtau,
                           uint32_t B, int64_t ld, hipStream_t s) {
    int64_t bs = 256;
    void *args[] = {&q, &qd, &tau, &qdd, &dq, &dqd, &dtau, &B, &ld, &bs};
    return launch_any(mb, rbamd::JitKind::FdDeriv, sizeof(T) == 8, B, false, s, args,
                      [&] { return no_generic(mb, "the dynamics derivatives run"); });
}

rbamd::JitKind vjp_kind(bool contact) {
    return contact ? rbamd::JitKind::RolloutContactVjp : rbamd::JitKind::RolloutVjp;
}
const char *vjp_name(bool contact) { return contact ? "rollout_contact_vjp" : "rollout_vjp"; }

// The rollouts' reverse-mode gradients (rollout_vjp_body.hip.hpp; contact: contact_vjp_body.hip.hpp, the
// same arguments): a model-specialised kernel only, SoA rows, as the derivatives above.
template <typename T>
hipError_t launch_rollout_vjp(const Multibody *mb, bool contact, const T *q, const T *qd, const T *tau_seq, T dt, int K, const T *gq,
                              const T *gqd, T *g_q0, T *g_qd0, T *g_tau, T *work, uint32_t B, int64_t ld,
                              hipStream_t s) {
    void *args[] = {&q, &qd, &tau_seq, &dt, &K, &gq, &gqd, &g_q0, &g_qd0, &g_tau, &work, &B, &ld};
    return launch_any(mb, vjp_kind(contact), sizeof(T) == 8, B, false, s, args,
                      [&] { return no_generic(mb, "the rollout gradient runs"); });
}

// Dynamics under external link wrenches (ext_body.hip.hpp): model-specialised kernels only, SoA
// rows, every model; fext has 6 n rows.
template <typename T>
hipError_t launch_ext(const Multibody *mb, bool fd, const T *q, const T *qd, const T *third, const T *fext, T *out,
                      uint32_t B, int64_t ld, hipStream_t s) {
    int64_t bs = 256;
    void *args[] = {&q, &qd, &third, &fext, &out, &B, &ld, &bs};
    return launch_any(mb, fd ? rbamd::JitKind::FdExt : rbamd::JitKind::RneaExt, sizeof(T) == 8, B, false, s, args,
                      [&] { return no_generic(mb, "the external-wrench dynamics run"); });
}

// Kinematics of every link (link_kin_body.hip.hpp): model-specialised kernels only, SoA rows, every
// model; pos has 3 n rows, rot 9 n, vel 6 n.
template <typename T>
hipError_t launch_link_pose(const Multibody *mb, const T *q, T *pos, T *rot, uint32_t B, int64_t ld, hipStream_t s) {
    int64_t bs = 256;
    void *args[] = {&q, &pos, &rot, &B, &ld, &bs};
    return launch_any(mb, rbamd::JitKind::LinkPose, sizeof(T) == 8, B, false, s, args,
                      [&] { return no_generic(mb, "the link kinematics run"); });
}

template <typename T>
hipError_t launch_link_vel(const Multibody *mb, const T *q, const T *qd, T *vel, uint32_t B, int64_t ld,
                           hipStream_t s) {
    int64_t bs = 256;
    void *args[] = {&q, &qd, &vel, &B, &ld, &bs};
    return launch_any(mb, rbamd::JitKind::LinkVel, sizeof(T) == 8, B, false, s, args,
                      [&] { return no_generic(mb, "the link kinematics run"); });
}

// Whole-body quantities (centroidal_body.hip.hpp): model-specialised kernels only, SoA rows, every
// model with a positive total mass; com has 3 rows, hg 6, energy 2, ag 6 n.
template <typename T>
hipError_t launch_com(const Multibody *mb, bool cmm, const T *q, T *out, uint32_t B, int64_t ld, hipStream_t s) {
    int64_t bs = 256;
    void *args[] = {&q, &out, &B, &ld, &bs};
    return launch_any(mb, cmm ? rbamd::JitKind::Cmm : rbamd::JitKind::Com, sizeof(T) == 8, B, false, s, args,
                      [&] { return no_generic(mb, "the centroidal kernels run"); });
}

template <typename T>
hipError_t launch_centroidal(const Multibody *mb, const T *q, const T *qd, T *com, T *hg, T *energy, uint32_t B,
                             int64_t ld, hipStream_t s) {
    int64_t bs = 256;
    void *args[] = {&q, &qd, &com, &hg, &energy, &B, &ld, &bs};
    return launch_any(mb, rbamd::JitKind::Centroidal, sizeof(T) == 8, B, false, s, args,
                      [&] { return no_generic(mb, "the centroidal kernels run"); });
}

// Compliant ground contact (contact_body.hip.hpp): model-specialised kernels only, SoA rows, every
// model that carries a contact set; fext has 6 n rows, cforce 3 P.
template <typename T>
hipError_t launch_contact_wrench(const Multibody *mb, const T *q, const T *qd, T *fext, T *cforce, uint32_t B,
                                 int64_t ld, hipStream_t s) {
    int64_t bs = 256;
    void *args[] = {&q, &qd, &fext, &cforce, &B, &ld, &bs};
    return launch_any(mb, rbamd::JitKind::ContactWrench, sizeof(T) == 8, B, false, s, args,
                      [&] { return no_generic(mb, "the contact kernels run"); });
}

template <typename T>
hipError_t launch_rollout_contact(const Multibody *mb, T *q, T *qd, const T *tau_seq, T dt, int K, T *traj, uint32_t B,
                                  int64_t ld, hipStream_t s) {
    void *args[] = {&q, &qd, &tau_seq, &dt, &K, &traj, &B, &ld};
    return launch_any(mb, rbamd::JitKind::RolloutContact, sizeof(T) == 8, B, false, s, args,
                      [&] { return no_generic(mb, "the contact kernels run"); });
}

constexpr int64_t kChunk = int64_t(1) << 28;  // per-launch batch cap: b * sizeof(T) < 2^32

int check_batch(const Multibody *mb, int64_t batch, int64_t ld) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (batch < 0) return set_err(RB_ERR_ARG, "negative batch");
    if (ld < batch) return set_err(RB_ERR_ARG, "leading dimension ld < batch");
    return RB_OK;
}

// Thread-local staging for the single-configuration ABI: one stream, one device
// buffer and one pinned host buffer per thread and device (never freed: HIP teardown
// order at process exit is not ours to control).
struct Staging {
    hipStream_t stream = nullptr;
    double *dbuf = nullptr;
    size_t dcap = 0;
    double *hbuf = nullptr;
    size_t hcap = 0;
};
thread_local std::map<int, Staging> t_staging;

int staging(size_t doubles, Staging **out) {
    int d = 0;
    hipError_t e = hipGetDevice(&d);
    if (e != hipSuccess) return hip_err(e, "hipGetDevice");
    Staging &s = t_staging[d];
    if (!s.stream) {
        if ((e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking)) != hipSuccess)
            return hip_err(e, "hipStreamCreate");
    }
    if (s.dcap < doubles) {
        if (s.dbuf) (void)hipFree(s.dbuf);
        s.dbuf = nullptr;
        s.dcap = 0;
        if ((e = hipMalloc(&s.dbuf, doubles * sizeof(double))) != hipSuccess) return hip_err(e, "hipMalloc");
        s.dcap = doubles;
    }
    if (s.hcap < doubles) {
        if (s.hbuf) (void)hipHostFree(s.hbuf);
        s.hbuf = nullptr;
        s.hcap = 0;
        if ((e = hipHostMalloc(&s.hbuf, doubles * sizeof(double), hipHostMallocDefault)) != hipSuccess)
            return hip_err(e, "hipHostMalloc");
        s.hcap = doubles;
    }
    *out = &s;
    return RB_OK;
}

// Host evaluation of one single-configuration query (host_eval.cpp) when the model and CPU
// allow it and the caller has not asked for the GPU (tuning single_gpu); `eval(out)` fills
// the result.  Returns the malloc'd result, or nullptr with *used = false to take the GPU.
template <typename F>
double *single_host(const Multibody *mb, const double *const *inputs, int nin, size_t nout, bool *used, F eval) {
    *used = false;
    if (!mb || rbamd::tuning().single_gpu != 0 || !rbamd::host_eval_supported(mb->model)) return nullptr;
    for (int k = 0; k < nin; ++k)
        if (!inputs[k]) { set_err(RB_ERR_NULL, "NULL input vector"); *used = true; return nullptr; }
    *used = true;
    double *res = static_cast<double *>(std::malloc(nout * sizeof(double)));
    if (!res) { set_err(RB_ERR_ARG, "out of host memory"); return nullptr; }
    if (!eval(res)) { std::free(res); *used = false; return nullptr; }
    return res;
}

// Runs one single-configuration query on the GPU: `nin` input vectors of n doubles,
// `nout` output doubles; `launch(dev_in, dev_out, stream)` enqueues the kernel.
template <typename F>
double *single_query(const Multibody *mb, const double *const *inputs, int nin, size_t nout, F launch) {
    if (!mb) { set_err(RB_ERR_NULL, "NULL Multibody handle"); return nullptr; }
    const int n = mb->model.n;
    for (int k = 0; k < nin; ++k)
        if (!inputs[k]) { set_err(RB_ERR_NULL, "NULL input vector"); return nullptr; }
    Staging *s = nullptr;
    const size_t total = (size_t)nin * n + nout;
    if (staging(total, &s) != RB_OK) return nullptr;
    for (int k = 0; k < nin; ++k) std::memcpy(s->hbuf + (size_t)k * n, inputs[k], n * sizeof(double));
    hipError_t e = hipMemcpyAsync(s->dbuf, s->hbuf, (size_t)nin * n * sizeof(double), hipMemcpyHostToDevice, s->stream);
    if (e != hipSuccess) { hip_err(e, "hipMemcpyAsync H2D"); return nullptr; }
    int rc = launch(s->dbuf, s->dbuf + (size_t)nin * n, s->stream);
    if (rc != RB_OK) return nullptr;
    e = hipMemcpyAsync(s->hbuf + (size_t)nin * n, s->dbuf + (size_t)nin * n, nout * sizeof(double), hipMemcpyDeviceToHost, s->stream);
    if (e != hipSuccess) { hip_err(e, "hipMemcpyAsync D2H"); return nullptr; }
    if ((e = hipStreamSynchronize(s->stream)) != hipSuccess) { hip_err(e, "hipStreamSynchronize"); return nullptr; }
    double *res = static_cast<double *>(std::malloc(nout * sizeof(double)));
    if (!res) { set_err(RB_ERR_ARG, "out of host memory"); return nullptr; }
    std::memcpy(res, s->hbuf + (size_t)nin * n, nout * sizeof(double));
    return res;
}

// One single-configuration query of the reference ABI: on the host where that is allowed
// (`host(out)`, single_host), else one GPU launch (`gpu(mdl, dev_in, dev_out, stream)`,
// single_query); `where` labels a failed launch.
template <typename Host, typename Gpu>
double *single_config(const Multibody *mb, std::initializer_list<const double *> inputs, size_t nout, const char *where,
                      Host host, Gpu gpu) {
    const double *const *in = inputs.begin();
    const int nin = (int)inputs.size();
    bool used = false;
    double *r = single_host(mb, in, nin, nout, &used, host);
    if (used) return r;
    return single_query(mb, in, nin, nout, [&](double *din, double *dout, hipStream_t s) {
        const double *mdl = nullptr;
        int rc = device_consts<double>(mb, &mdl);
        if (rc) return rc;
        hipError_t e = gpu(mdl, din, dout, s);
        return e == hipSuccess ? RB_OK : hip_err(e, where);
    });
}

template <typename T, typename L>
int chunked(int64_t batch, L &&one) {
    for (int64_t b0 = 0; b0 < batch; b0 += kChunk) {
        const int64_t nb = batch - b0 < kChunk ? batch - b0 : kChunk;
        int rc = one(b0, (uint32_t)nb);
        if (rc != RB_OK) return rc;
    }
    return RB_OK;
}

int no_null(std::initializer_list<const void *> arrays) {
    for (const void *p : arrays)
        if (!p) return set_err(RB_ERR_NULL, "NULL array");
    return RB_OK;
}

// Where configuration b0 (a multiple of 256) starts in the arrays of one call: at(p, rows) for an
// array of `rows` rows per configuration -- b0 elements along SoA rows, b0 * rows into the tiled
// layout; a NULL (optional) array stays NULL.
struct ChunkAt {
    int64_t b0;
    bool tiled;
    template <typename P>
    P *operator()(P *p, int64_t rows) const {
        return p ? p + b0 * (tiled ? rows : 1) : nullptr;
    }
};

// The spine of every batched entry point.  Argument errors are reported in this order: handle,
// batch, ld (check_batch), then the entry point's own arrays (`args_ok`: its NULL check, and
// whatever else it refuses), then the device.  `launch(mdl, at, nb)` enqueues the nb (at most
// kChunk) configurations that start where `at` points; `where` labels its failure.
template <typename T, typename Check, typename Launch>
int batch_call(const Multibody *mb, int64_t batch, int64_t ld, bool tiled, Check args_ok, const char *where,
               Launch launch) {
    int rc = check_batch(mb, batch, tiled ? batch : ld);
    if (rc) return rc;
    if (batch == 0) return RB_OK;
    if ((rc = args_ok())) return rc;
    const T *mdl = nullptr;
    if ((rc = device_consts<T>(mb, &mdl))) return rc;
    return chunked<T>(batch, [&](int64_t b0, uint32_t nb) {
        hipError_t e = launch(mdl, ChunkAt{b0, tiled}, nb);
        return e == hipSuccess ? RB_OK : hip_err(e, where);
    });
}

template <typename T>
int rnea_batch(const Multibody *mb, const T *q, const T *qd, const T *qdd, T *tau, int64_t batch,
               int64_t ld, void *stream, bool tiled = false) {
    return batch_call<T>(mb, batch, ld, tiled, [&] { return no_null({q, qd, qdd, tau}); }, "rnea launch",
                         [&](const T *mdl, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;
        return launch_rnea_any<T>(mb, mdl, at(q, n), at(qd, n), at(qdd, n), at(tau, n), nb, ld, (hipStream_t)stream,
                                  tiled);
    });
}

template <typename T>
int fd_batch(const Multibody *mb, const T *q, const T *qd, const T *tau, T *qdd, int64_t batch,
             int64_t ld, void *stream, bool tiled = false) {
    return batch_call<T>(mb, batch, ld, tiled, [&] { return no_null({q, qd, tau, qdd}); }, "aba launch",
                         [&](const T *mdl, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;
        return launch_fd_any<T>(mb, mdl, at(q, n), at(qd, n), at(tau, n), at(qdd, n), nb, ld, (hipStream_t)stream,
                                tiled);
    });
}

template <typename T>
int idfd_batch(const Multibody *mb, const T *q, const T *qd, const T *qdd, const T *tau_in, T *tau, T *qdd_out,
               int64_t batch, int64_t ld, void *stream, bool tiled = false) {
    auto args_ok = [&] {
        if (int rc = no_null({q, qd, qdd, tau_in, tau, qdd_out})) return rc;
        // outputs must not overlap the inputs (the kernel reads tau_in after storing tau); the exact
        // aliases a caller is likely to pass -- tau_in as tau, qdd as qdd_out -- are refused here
        for (const T *o : {(const T *)tau, (const T *)qdd_out})
            for (const T *i : {q, qd, qdd, tau_in})
                if (o == i) return set_err(RB_ERR_ARG, "rnea_fd: an output array is also an input (no in-place form)");
        if (tau == qdd_out) return set_err(RB_ERR_ARG, "rnea_fd: tau and qdd_out are the same array");
        return (int)RB_OK;
    };
    return batch_call<T>(mb, batch, ld, tiled, args_ok, "rnea_fd launch", [&](const T *mdl, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;
        return launch_idfd_any<T>(mb, mdl, at(q, n), at(qd, n), at(qdd, n), at(tau_in, n), at(tau, n), at(qdd_out, n),
                                  nb, ld, (hipStream_t)stream, tiled);
    });
}

// The external-wrench entry points' own argument checks: every array present, the output none of
// the inputs.  op: "rnea_ext" / "fd_ext".
template <typename T>
int ext_args_ok(const char *op, std::initializer_list<const T *> in, const T *out) {
    if (!out) return set_err(RB_ERR_NULL, "NULL array");
    for (const T *p : in)
        if (!p) return set_err(RB_ERR_NULL, "NULL array");
    for (const T *p : in)
        if (p == out) return set_err(RB_ERR_ARG, std::string(op) + ": an output array is also an input (no in-place form)");
    return RB_OK;
}

// third: qdd (rnea_ext, out = tau) or tau (fd_ext, out = qdd)
template <typename T>
int ext_batch(const Multibody *mb, bool fd, const T *q, const T *qd, const T *third, const T *fext, T *out,
              int64_t batch, int64_t ld, void *stream) {
    auto args_ok = [&] { return ext_args_ok<T>(fd ? "fd_ext" : "rnea_ext", {q, qd, third, fext}, out); };
    return batch_call<T>(mb, batch, ld, false, args_ok, fd ? "fd_ext launch" : "rnea_ext launch",
                         [&](const T *, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;
        return launch_ext<T>(mb, fd, at(q, n), at(qd, n), at(third, n), at(fext, 6 * n), at(out, n), nb, ld,
                             (hipStream_t)stream);
    });
}

// The inverse dynamics' reverse-mode gradient (rnea_vjp_body.hip.hpp): model-specialised kernels only,
// SoA rows, every model.  wrench = false: the plain RNEA's kernel, which has no wrench parameters (fext and
// g_fext are not looked at).
template <typename T>
hipError_t launch_rnea_vjp(const Multibody *mb, bool wrench, const T *q, const T *qd, const T *qdd, const T *fext, const T *w,
                           T *g_q, T *g_qd, T *g_qdd, T *g_fext, uint32_t B, int64_t ld, hipStream_t s) {
    int64_t bs = 256;
    auto refuse = [&] { return no_generic(mb, "the inverse dynamics' gradient runs"); };
    if (wrench) {
        void *args[] = {&q, &qd, &qdd, &fext, &w, &g_q, &g_qd, &g_qdd, &g_fext, &B, &ld, &bs};
        return launch_any(mb, rbamd::JitKind::RneaVjpExt, sizeof(T) == 8, B, false, s, args, refuse);
    }
    void *args[] = {&q, &qd, &qdd, &w, &g_q, &g_qd, &g_qdd, &B, &ld, &bs};
    return launch_any(mb, rbamd::JitKind::RneaVjp, sizeof(T) == 8, B, false, s, args, refuse);
}

// rnea_vjp's own argument checks: every array present, no output that is also an input or another
// output.  wrench: the form with fext / g_fext (else both are NULL and not looked at).  optional: the
// single-configuration form, where fext NULL selects the plain RNEA (g_fext must then be NULL too) and
// g_fext alone may be NULL (not evaluated).
template <typename T>
int rnea_vjp_args_ok(bool wrench, bool optional, const T *q, const T *qd, const T *qdd, const T *fext, const T *w,
                     const T *g_q, const T *g_qd, const T *g_qdd, const T *g_fext) {
    for (const T *p : {q, qd, qdd, w, g_q, g_qd, g_qdd})
        if (!p) return set_err(RB_ERR_NULL, "NULL array");
    if (wrench && !optional && (!fext || !g_fext)) return set_err(RB_ERR_NULL, "NULL array");
    if (g_fext && !fext) return set_err(RB_ERR_ARG, "rnea_vjp: g_fext without fext (the plain RNEA has no wrench)");
    const T *out[] = {g_q, g_qd, g_qdd, g_fext};
    for (int a = 0; a < 4; ++a) {
        if (!out[a]) continue;
        for (const T *i : {q, qd, qdd, fext, w})
            if (out[a] == i) return set_err(RB_ERR_ARG, "rnea_vjp: an output array is also an input");
        for (int b = 0; b < a; ++b)
            if (out[a] == out[b]) return set_err(RB_ERR_ARG, "rnea_vjp: two outputs are the same array");
    }
    return RB_OK;
}

// wrench = false: multibody_rnea_vjp_plain_batch_* (fext, g_fext NULL)
template <typename T>
int rnea_vjp_batch(const Multibody *mb, bool wrench, const T *q, const T *qd, const T *qdd, const T *fext, const T *w,
                   T *g_q, T *g_qd, T *g_qdd, T *g_fext, int64_t batch, int64_t ld, void *stream) {
    if (!wrench) {  // the plain family has no wrench arrays: the kernel is chosen by the family alone
        fext = nullptr;
        g_fext = nullptr;
    }
    auto args_ok = [&] { return rnea_vjp_args_ok<T>(wrench, false, q, qd, qdd, fext, w, g_q, g_qd, g_qdd, g_fext); };
    return batch_call<T>(mb, batch, ld, false, args_ok, "rnea_vjp launch", [&](const T *, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;
        return launch_rnea_vjp<T>(mb, wrench, at(q, n), at(qd, n), at(qdd, n), at(fext, 6 * n), at(w, n), at(g_q, n),
                                  at(g_qd, n), at(g_qdd, n), at(g_fext, 6 * n), nb, ld, (hipStream_t)stream);
    });
}

// The forward dynamics' reverse-mode gradient (fd_vjp_body.hip.hpp): model-specialised kernels only, SoA
// rows, every model.  wrench = false: the kernel without wrench parameters (fext and g_fext are not
// looked at).
template <typename T>
hipError_t launch_fd_vjp(const Multibody *mb, bool wrench, const T *q, const T *qd, const T *tau, const T *fext, const T *w,
                         T *qdd, T *g_q, T *g_qd, T *g_tau, T *g_fext, uint32_t B, int64_t ld, hipStream_t s) {
    int64_t bs = 256;
    auto refuse = [&] { return no_generic(mb, "the forward dynamics' gradient runs"); };
    if (wrench) {
        void *args[] = {&q, &qd, &tau, &fext, &w, &qdd, &g_q, &g_qd, &g_tau, &g_fext, &B, &ld, &bs};
        return launch_any(mb, rbamd::JitKind::FdVjpExt, sizeof(T) == 8, B, false, s, args, refuse);
    }
    void *args[] = {&q, &qd, &tau, &w, &qdd, &g_q, &g_qd, &g_tau, &B, &ld, &bs};
    return launch_any(mb, rbamd::JitKind::FdVjp, sizeof(T) == 8, B, false, s, args, refuse);
}

// fd_vjp's own argument checks, rnea_vjp_args_ok's with qdd among the outputs.
template <typename T>
int fd_vjp_args_ok(bool wrench, bool optional, const T *q, const T *qd, const T *tau, const T *fext, const T *w,
                   const T *qdd, const T *g_q, const T *g_qd, const T *g_tau, const T *g_fext) {
    for (const T *p : {q, qd, tau, w, qdd, g_q, g_qd, g_tau})
        if (!p) return set_err(RB_ERR_NULL, "NULL array");
    if (wrench && !optional && (!fext || !g_fext)) return set_err(RB_ERR_NULL, "NULL array");
    if (g_fext && !fext) return set_err(RB_ERR_ARG, "fd_vjp: g_fext without fext (the plain forward dynamics has no wrench)");
    const T *out[] = {qdd, g_q, g_qd, g_tau, g_fext};
    for (int a = 0; a < 5; ++a) {
        if (!out[a]) continue;
        for (const T *i : {q, qd, tau, fext, w})
            if (out[a] == i) return set_err(RB_ERR_ARG, "fd_vjp: an output array is also an input");
        for (int b = 0; b < a; ++b)
            if (out[a] == out[b]) return set_err(RB_ERR_ARG, "fd_vjp: two outputs are the same array");
    }
    return RB_OK;
}

// wrench = false: multibody_fd_vjp_plain_batch_* (fext, g_fext NULL)
template <typename T>
int fd_vjp_batch(const Multibody *mb, bool wrench, const T *q, const T *qd, const T *tau, const T *fext, const T *w,
                 T *qdd, T *g_q, T *g_qd, T *g_tau, T *g_fext, int64_t batch, int64_t ld, void *stream) {
    if (!wrench) {  // the plain family has no wrench arrays: the kernel is chosen by the family alone
        fext = nullptr;
        g_fext = nullptr;
    }
    auto args_ok = [&] { return fd_vjp_args_ok<T>(wrench, false, q, qd, tau, fext, w, qdd, g_q, g_qd, g_tau, g_fext); };
    return batch_call<T>(mb, batch, ld, false, args_ok, "fd_vjp launch", [&](const T *, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;
        return launch_fd_vjp<T>(mb, wrench, at(q, n), at(qd, n), at(tau, n), at(fext, 6 * n), at(w, n), at(qdd, n),
                                at(g_q, n), at(g_qd, n), at(g_tau, n), at(g_fext, 6 * n), nb, ld, (hipStream_t)stream);
    });
}

// RB_ERR_UNSUPPORTED (with the condition that failed) when `kind` has no kernel for this model.
int deriv_supported(const Multibody *mb, rbamd::JitKind kind) {
    const std::string why = rbamd::jit_kind_unsupported(mb->model, kind);
    return why.empty() ? (int)RB_OK : set_err(RB_ERR_UNSUPPORTED, why);
}

// The derivative entry points' own argument checks: inputs present, at least one output, no
// output that is also an input or another output, a model in scope.
template <typename T>
int deriv_args_ok(const Multibody *mb, rbamd::JitKind kind, const char *name, std::initializer_list<const T *> in,
                  std::initializer_list<const T *> out) {
    for (const T *p : in)
        if (!p) return set_err(RB_ERR_NULL, "NULL array");
    bool any = false;
    for (const T *o : out) any = any || o != nullptr;
    if (!any) return set_err(RB_ERR_NULL, std::string(name) + ": every output is NULL");
    for (const T *const *o = out.begin(); o != out.end(); ++o) {
        if (!*o) continue;
        for (const T *i : in)
            if (*o == i) return set_err(RB_ERR_ARG, std::string(name) + ": an output array is also an input");
        for (const T *const *o2 = out.begin(); o2 != o; ++o2)
            if (*o == *o2) return set_err(RB_ERR_ARG, std::string(name) + ": two outputs are the same array");
    }
    return deriv_supported(mb, kind);
}

template <typename T>
int rnea_deriv_batch(const Multibody *mb, const T *q, const T *qd, const T *qdd, T *dq, T *dqd, int64_t batch,
                     int64_t ld, void *stream) {
    auto args_ok = [&] {
        return deriv_args_ok<T>(mb, rbamd::JitKind::RneaDeriv, "rnea_deriv", {q, qd, qdd}, {dq, dqd});
    };
    return batch_call<T>(mb, batch, ld, false, args_ok, "rnea_deriv launch", [&](const T *, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n, nn = n * n;
        return launch_rnea_deriv<T>(mb, at(q, n), at(qd, n), at(qdd, n), at(dq, nn), at(dqd, nn), nb, ld,
                                    (hipStream_t)stream);
    });
}

template <typename T>
int fd_deriv_batch(const Multibody *mb, const T *q, const T *qd, const T *tau, T *qdd, T *dq, T *dqd, T *dtau,
                   int64_t batch, int64_t ld, void *stream) {
    auto args_ok = [&] {
        return deriv_args_ok<T>(mb, rbamd::JitKind::FdDeriv, "fd_deriv", {q, qd, tau}, {qdd, dq, dqd, dtau});
    };
    return batch_call<T>(mb, batch, ld, false, args_ok, "fd_deriv launch", [&](const T *, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n, nn = n * n;
        return launch_fd_deriv<T>(mb, at(q, n), at(qd, n), at(tau, n), at(qdd, n), at(dq, nn), at(dqd, nn),
                                  at(dtau, nn), nb, ld, (hipStream_t)stream);
    });
}

// The link-kinematics entry points' own argument checks: every array present, no output that is
// also an input or the other output.  vel: link_vel (else link_pose); every model is in scope.
template <typename T>
int link_kin_args_ok(const Multibody *mb, bool vel, std::initializer_list<const T *> in,
                     std::initializer_list<const T *> out) {
    for (const T *p : out)
        if (!p) return set_err(RB_ERR_NULL, "NULL array");
    return deriv_args_ok<T>(mb, vel ? rbamd::JitKind::LinkVel : rbamd::JitKind::LinkPose, vel ? "link_vel" : "link_pose",
                            in, out);
}

template <typename T>
int link_pose_batch(const Multibody *mb, const T *q, T *pos, T *rot, int64_t batch, int64_t ld, void *stream) {
    auto args_ok = [&] { return link_kin_args_ok<T>(mb, false, {q}, {pos, rot}); };
    return batch_call<T>(mb, batch, ld, false, args_ok, "link_pose launch", [&](const T *, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;
        return launch_link_pose<T>(mb, at(q, n), at(pos, 3 * n), at(rot, 9 * n), nb, ld, (hipStream_t)stream);
    });
}

template <typename T>
int link_vel_batch(const Multibody *mb, const T *q, const T *qd, T *vel, int64_t batch, int64_t ld, void *stream) {
    auto args_ok = [&] { return link_kin_args_ok<T>(mb, true, {q, qd}, {vel}); };
    return batch_call<T>(mb, batch, ld, false, args_ok, "link_vel launch", [&](const T *, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;
        return launch_link_vel<T>(mb, at(q, n), at(qd, n), at(vel, 6 * n), nb, ld, (hipStream_t)stream);
    });
}

// The centroidal entry points' own argument checks: every array present, no output that is also an
// input or another output, a model with mass.  which: 0 com, 1 centroidal, 2 cmm.
rbamd::JitKind centroidal_kind(int which) {
    return which == 0 ? rbamd::JitKind::Com : which == 1 ? rbamd::JitKind::Centroidal : rbamd::JitKind::Cmm;
}
const char *centroidal_name(int which) { return which == 0 ? "com" : which == 1 ? "centroidal" : "cmm"; }

template <typename T>
int centroidal_args_ok(const Multibody *mb, int which, std::initializer_list<const T *> in,
                       std::initializer_list<const T *> out) {
    for (const T *p : out)
        if (!p) return set_err(RB_ERR_NULL, "NULL array");
    return deriv_args_ok<T>(mb, centroidal_kind(which), centroidal_name(which), in, out);
}

// com (cmm = false, out [3]) / cmm (out [6 n])
template <typename T>
int com_batch(const Multibody *mb, bool cmm, const T *q, T *out, int64_t batch, int64_t ld, void *stream) {
    auto args_ok = [&] { return centroidal_args_ok<T>(mb, cmm ? 2 : 0, {q}, {out}); };
    return batch_call<T>(mb, batch, ld, false, args_ok, cmm ? "cmm launch" : "com launch",
                         [&](const T *, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;
        return launch_com<T>(mb, cmm, at(q, n), at(out, cmm ? 6 * n : 3), nb, ld, (hipStream_t)stream);
    });
}

template <typename T>
int centroidal_batch(const Multibody *mb, const T *q, const T *qd, T *com, T *hg, T *energy, int64_t batch, int64_t ld,
                     void *stream) {
    auto args_ok = [&] { return centroidal_args_ok<T>(mb, 1, {q, qd}, {com, hg, energy}); };
    return batch_call<T>(mb, batch, ld, false, args_ok, "centroidal launch", [&](const T *, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;
        return launch_centroidal<T>(mb, at(q, n), at(qd, n), at(com, 3), at(hg, 6), at(energy, 2), nb, ld,
                                    (hipStream_t)stream);
    });
}

// The contact entry points' own argument checks: every array present, no output (the rollout's
// state included) that is also an input or another output, a model that carries a contact set.
template <typename T>
int contact_args_ok(const Multibody *mb, bool rollout, std::initializer_list<const T *> in,
                    std::initializer_list<const T *> out) {
    for (const T *p : in)
        if (!p) return set_err(RB_ERR_NULL, "NULL array");
    for (const T *p : out)
        if (!p) return set_err(RB_ERR_NULL, "NULL array");
    return deriv_args_ok<T>(mb, rollout ? rbamd::JitKind::RolloutContact : rbamd::JitKind::ContactWrench,
                            rollout ? "rollout_contact" : "contact_wrench", in, out);
}

// The rollouts' step count, after handle / batch / ld and before the empty-batch return; *done: K == 0.
int rollout_steps(const Multibody *mb, int64_t batch, int64_t ld, int K, bool *done) {
    *done = false;
    if (int rc = check_batch(mb, batch, ld)) return rc;
    if (K < 0) return set_err(RB_ERR_ARG, "negative step count");
    *done = K == 0;
    return RB_OK;
}

template <typename T>
int contact_wrench_batch(const Multibody *mb, const T *q, const T *qd, T *fext, T *cforce, int64_t batch, int64_t ld,
                         void *stream) {
    auto args_ok = [&] { return contact_args_ok<T>(mb, false, {q, qd}, {fext, cforce}); };
    return batch_call<T>(mb, batch, ld, false, args_ok, "contact_wrench launch", [&](const T *, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n, np = mb->model.contacts.n_points;
        return launch_contact_wrench<T>(mb, at(q, n), at(qd, n), at(fext, 6 * n), at(cforce, 3 * np), nb, ld,
                                        (hipStream_t)stream);
    });
}

template <typename T>
int rollout_contact_batch(const Multibody *mb, T *q, T *qd, const T *tau_seq, double dt, int K, T *traj, int64_t batch,
                          int64_t ld, void *stream) {
    bool done = false;
    if (int rc = rollout_steps(mb, batch, ld, K, &done)) return rc;
    if (done) return RB_OK;
    auto args_ok = [&] { return contact_args_ok<T>(mb, true, {tau_seq}, {q, qd, traj}); };
    return batch_call<T>(mb, batch, ld, false, args_ok, "rollout_contact launch", [&](const T *, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;  // tau_seq and traj: K * n rows
        return launch_rollout_contact<T>(mb, at(q, n), at(qd, n), at(tau_seq, K * n), (T)dt, K, at(traj, K * n), nb, ld,
                                         (hipStream_t)stream);
    });
}

template <typename T>
int rollout_batch(const Multibody *mb, T *q, T *qd, const T *tau_seq, double dt, int K, T *traj, int64_t batch,
                  int64_t ld, void *stream) {
    // the step count is checked after handle / batch / ld and before the empty-batch return, so
    // check_batch runs here and once more (cheap, same answer) inside batch_call
    int rc = check_batch(mb, batch, ld);
    if (rc) return rc;
    if (K < 0) return set_err(RB_ERR_ARG, "negative step count");
    if (K == 0) return RB_OK;
    return batch_call<T>(mb, batch, ld, false, [&] { return no_null({q, qd, tau_seq}); }, "rollout launch",
                         [&](const T *mdl, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;  // tau_seq and traj: K * n rows, SoA only
        return launch_rollout_any<T>(mb, mdl, at(q, n), at(qd, n), at(tau_seq, K * n), (T)dt, K, at(traj, K * n), nb, ld,
                                     (hipStream_t)stream);
    });
}

// The rollout gradients' checks after handle / batch / ld and the empty-batch return: the step
// count, then (`arrays`) every array present, no output or the workspace aliased, a model in scope
// (contact: one that carries a contact set, checked just before the scope).
int vjp_steps_ok(bool contact, int K) {
    if (K < 0) return set_err(RB_ERR_ARG, "negative step count");
    if (K == 0) return set_err(RB_ERR_ARG, std::string(vjp_name(contact)) + ": K == 0 steps, nothing to differentiate");
    return RB_OK;
}

template <typename T>
int vjp_args_ok(const Multibody *mb, bool contact, std::initializer_list<const T *> in,
                std::initializer_list<const T *> out) {
    for (const T *p : out)
        if (!p) return set_err(RB_ERR_NULL, "NULL array");
    return deriv_args_ok<T>(mb, vjp_kind(contact), vjp_name(contact), in, out);
}

template <typename T>
int rollout_vjp_batch(const Multibody *mb, bool contact, const T *q, const T *qd, const T *tau_seq, double dt, int K, const T *gq,
                      const T *gqd, T *g_q0, T *g_qd0, T *g_tau, T *work, int64_t batch, int64_t ld, void *stream) {
    auto args_ok = [&] {
        if (int rc = vjp_steps_ok(contact, K)) return rc;
        return vjp_args_ok<T>(mb, contact, {q, qd, tau_seq, gq, gqd}, {g_q0, g_qd0, g_tau, work});
    };
    return batch_call<T>(mb, batch, ld, false, args_ok, contact ? "rollout_contact_vjp launch" : "rollout_vjp launch",
                         [&](const T *, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;  // tau_seq, gq, gqd, g_tau: K * n rows; work: 2 K n
        return launch_rollout_vjp<T>(mb, contact, at(q, n), at(qd, n), at(tau_seq, K * n), (T)dt, K, at(gq, K * n),
                                     at(gqd, K * n), at(g_q0, n), at(g_qd0, n), at(g_tau, K * n), at(work, 2 * K * n), nb,
                                     ld, (hipStream_t)stream);
    });
}

template <typename T>
int crba_batch(const Multibody *mb, const T *q, T *H, int64_t batch, int64_t ld, void *stream, bool tiled = false) {
    return batch_call<T>(mb, batch, ld, tiled, [&] { return no_null({q, H}); }, "crba launch",
                         [&](const T *mdl, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;
        return launch_crba_any<T>(mb, mdl, at(q, n), at(H, n * n), nb, ld, (hipStream_t)stream, tiled);
    });
}

template <typename T>
int kin_batch(const Multibody *mb, bool jac, const T *q, T *out, int64_t batch, int64_t ld, void *stream,
              bool tiled = false) {
    return batch_call<T>(mb, batch, ld, tiled, [&] { return no_null({q, out}); }, jac ? "jac launch" : "fwd_kin launch",
                         [&](const T *mdl, ChunkAt at, uint32_t nb) {
        const int n = mb->model.n;
        return launch_kin_any<T>(mb, jac, mdl, at(q, n), at(out, jac ? 6 * n : 3), nb, ld, (hipStream_t)stream, tiled);
    });
}

Multibody *new_from_text(const std::string &xml, unsigned flags = 0) {
    try {
        return make(rbamd::Model::from_urdf_text(xml, flags));
    } catch (const std::exception &ex) {
        set_err(RB_ERR_URDF, ex.what());
        return nullptr;
    }
}

}  // namespace

namespace {
// The blocking host-pointer forms: SoA rows x[j * batch + b] in host memory, copied to a scratch
// device buffer on a private stream, evaluated by the batched kernels, copied back.  NIN inputs
// of n rows; NOUT outputs of rows[k] rows, a NULL one skipped where null_outputs allows it (it
// takes no scratch: the device offsets depend on which outputs are present).  check() is the
// entry point's own argument check, after the handle / batch / NULL checks and before any device
// work; launch(d_in[], d_out[], stream) gets the device arrays (NULL for a skipped output).
// host_call_rows: inputs of in_rows[k] rows, and `scratch_rows` more rows of device scratch handed to
// launch as d_out[NOUT] (a workspace no host array stands behind).
template <typename T, int NIN, int NOUT, typename Check, typename Launch>
int host_call_rows(const Multibody *mb, const T *const (&in)[NIN], const int64_t (&in_rows)[NIN], T *const (&out)[NOUT],
                   const int64_t (&rows)[NOUT], int64_t scratch_rows, bool null_outputs, int64_t batch, Check check,
                   Launch launch) {
    int rc = check_batch(mb, batch, batch);
    if (rc) return rc;
    if (batch == 0) return RB_OK;
    for (const T *p : in)
        if (!p) return set_err(RB_ERR_NULL, "NULL array");
    for (const T *p : out)
        if (!p && !null_outputs) return set_err(RB_ERR_NULL, "NULL array");
    if ((rc = check())) return rc;
    size_t total = 0, in_at[NIN], at[NOUT + 1];
    for (int k = 0; k < NIN; ++k) {
        in_at[k] = total;
        total += (size_t)in_rows[k] * (size_t)batch;
    }
    for (int k = 0; k < NOUT; ++k) {
        at[k] = total;
        if (out[k]) total += (size_t)rows[k] * (size_t)batch;
    }
    at[NOUT] = total;
    total += (size_t)scratch_rows * (size_t)batch;
    T *d = nullptr;
    hipStream_t s = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) return hip_err(e, "hipStreamCreate");
    e = hipMallocAsync((void **)&d, total * sizeof(T), s);
    if (e != hipSuccess) { (void)hipStreamDestroy(s); return hip_err(e, "hipMallocAsync"); }
    T *din[NIN], *dout[NOUT + 1];
    for (int k = 0; k < NIN; ++k) din[k] = d + in_at[k];
    for (int k = 0; k < NOUT; ++k) dout[k] = out[k] ? d + at[k] : nullptr;
    dout[NOUT] = scratch_rows ? d + at[NOUT] : nullptr;
    for (int k = 0; k < NIN && e == hipSuccess; ++k)
        e = hipMemcpyAsync(din[k], in[k], (size_t)in_rows[k] * (size_t)batch * sizeof(T), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) rc = launch(din, dout, s);
    else rc = hip_err(e, "hipMemcpyAsync H2D");
    for (int k = 0; k < NOUT && rc == RB_OK; ++k) {
        if (!out[k]) continue;
        e = hipMemcpyAsync(out[k], dout[k], (size_t)rows[k] * (size_t)batch * sizeof(T), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) rc = hip_err(e, "hipMemcpyAsync D2H");
    }
    (void)hipFreeAsync(d, s);
    e = hipStreamSynchronize(s);
    if (rc == RB_OK && e != hipSuccess) rc = hip_err(e, "hipStreamSynchronize");
    (void)hipStreamDestroy(s);
    return rc;
}

template <typename T, int NIN, int NOUT, typename Check, typename Launch>
int host_call(const Multibody *mb, const T *const (&in)[NIN], T *const (&out)[NOUT], const int64_t (&rows)[NOUT],
              bool null_outputs, int64_t batch, Check check, Launch launch) {
    int64_t in_rows[NIN];
    for (int64_t &r : in_rows) r = mb ? mb->model.n : 0;
    return host_call_rows<T, NIN, NOUT>(mb, in, in_rows, out, rows, 0, null_outputs, batch, check, launch);
}

const auto no_check = [] { return (int)RB_OK; };

template <typename T>
int rnea_host(const Multibody *mb, const T *q, const T *qd, const T *qdd, T *tau, int64_t batch) {
    const int64_t n = mb ? mb->model.n : 0;
    return host_call<T, 3, 1>(mb, {q, qd, qdd}, {tau}, {n}, false, batch, no_check, [&](T **i, T **o, hipStream_t s) {
        return rnea_batch<T>(mb, i[0], i[1], i[2], o[0], batch, batch, s);
    });
}
template <typename T>
int fd_host(const Multibody *mb, const T *q, const T *qd, const T *tau, T *qdd, int64_t batch) {
    const int64_t n = mb ? mb->model.n : 0;
    return host_call<T, 3, 1>(mb, {q, qd, tau}, {qdd}, {n}, false, batch, no_check, [&](T **i, T **o, hipStream_t s) {
        return fd_batch<T>(mb, i[0], i[1], i[2], o[0], batch, batch, s);
    });
}
template <typename T>
int idfd_host(const Multibody *mb, const T *q, const T *qd, const T *qdd, const T *tau_in, T *tau, T *qdd_out,
              int64_t batch) {
    const int64_t n = mb ? mb->model.n : 0;
    return host_call<T, 4, 2>(mb, {q, qd, qdd, tau_in}, {tau, qdd_out}, {n, n}, false, batch, no_check,
                              [&](T **i, T **o, hipStream_t s) {
        return idfd_batch<T>(mb, i[0], i[1], i[2], i[3], o[0], o[1], batch, batch, s);
    });
}

template <typename T>
int rnea_deriv_host(const Multibody *mb, const T *q, const T *qd, const T *qdd, T *dq, T *dqd, int64_t batch) {
    const int64_t nn = mb ? (int64_t)mb->model.n * mb->model.n : 0;
    return host_call<T, 3, 2>(
        mb, {q, qd, qdd}, {dq, dqd}, {nn, nn}, true, batch,
        [&] { return deriv_args_ok<T>(mb, rbamd::JitKind::RneaDeriv, "rnea_deriv", {q, qd, qdd}, {dq, dqd}); },
        [&](T **i, T **o, hipStream_t s) {
            return rnea_deriv_batch<T>(mb, i[0], i[1], i[2], o[0], o[1], batch, batch, s);
        });
}

template <typename T>
int fd_deriv_host(const Multibody *mb, const T *q, const T *qd, const T *tau, T *qdd, T *dq, T *dqd, T *dtau,
                  int64_t batch) {
    const int64_t n = mb ? mb->model.n : 0, nn = n * n;
    return host_call<T, 3, 4>(
        mb, {q, qd, tau}, {qdd, dq, dqd, dtau}, {n, nn, nn, nn}, true, batch,
        [&] { return deriv_args_ok<T>(mb, rbamd::JitKind::FdDeriv, "fd_deriv", {q, qd, tau}, {qdd, dq, dqd, dtau}); },
        [&](T **i, T **o, hipStream_t s) {
            return fd_deriv_batch<T>(mb, i[0], i[1], i[2], o[0], o[1], o[2], o[3], batch, batch, s);
        });
}

template <typename T>
int ext_host(const Multibody *mb, bool fd, const T *q, const T *qd, const T *third, const T *fext, T *out,
             int64_t batch) {
    const int64_t n = mb ? mb->model.n : 0;
    return host_call_rows<T, 4, 1>(mb, {q, qd, third, fext}, {n, n, n, 6 * n}, {out}, {n}, 0, false, batch, no_check,
                                   [&](T **i, T **o, hipStream_t s) {
        return ext_batch<T>(mb, fd, i[0], i[1], i[2], i[3], o[0], batch, batch, s);
    });
}

// wrench = false: multibody_rnea_vjp_plain_batch_host_* (fext, g_fext NULL)
template <typename T>
int rnea_vjp_host(const Multibody *mb, bool wrench, const T *q, const T *qd, const T *qdd, const T *fext, const T *w,
                  T *g_q, T *g_qd, T *g_qdd, T *g_fext, int64_t batch) {
    const int64_t n = mb ? mb->model.n : 0;
    auto check = [&] { return rnea_vjp_args_ok<T>(wrench, false, q, qd, qdd, fext, w, g_q, g_qd, g_qdd, g_fext); };
    if (!wrench)
        return host_call_rows<T, 4, 3>(mb, {q, qd, qdd, w}, {n, n, n, n}, {g_q, g_qd, g_qdd}, {n, n, n}, 0, false, batch,
                                       check, [&](T **i, T **o, hipStream_t s) {
            return rnea_vjp_batch<T>(mb, false, i[0], i[1], i[2], nullptr, i[3], o[0], o[1], o[2], nullptr, batch, batch, s);
        });
    return host_call_rows<T, 5, 4>(mb, {q, qd, qdd, fext, w}, {n, n, n, 6 * n, n}, {g_q, g_qd, g_qdd, g_fext},
                                   {n, n, n, 6 * n}, 0, false, batch, check, [&](T **i, T **o, hipStream_t s) {
        return rnea_vjp_batch<T>(mb, true, i[0], i[1], i[2], i[3], i[4], o[0], o[1], o[2], o[3], batch, batch, s);
    });
}

// wrench = false: multibody_fd_vjp_plain_batch_host_* (fext, g_fext NULL)
template <typename T>
int fd_vjp_host(const Multibody *mb, bool wrench, const T *q, const T *qd, const T *tau, const T *fext, const T *w,
                T *qdd, T *g_q, T *g_qd, T *g_tau, T *g_fext, int64_t batch) {
    const int64_t n = mb ? mb->model.n : 0;
    auto check = [&] { return fd_vjp_args_ok<T>(wrench, false, q, qd, tau, fext, w, qdd, g_q, g_qd, g_tau, g_fext); };
    if (!wrench)
        return host_call_rows<T, 4, 4>(mb, {q, qd, tau, w}, {n, n, n, n}, {qdd, g_q, g_qd, g_tau}, {n, n, n, n}, 0, false,
                                       batch, check, [&](T **i, T **o, hipStream_t s) {
            return fd_vjp_batch<T>(mb, false, i[0], i[1], i[2], nullptr, i[3], o[0], o[1], o[2], o[3], nullptr, batch, batch, s);
        });
    return host_call_rows<T, 5, 5>(mb, {q, qd, tau, fext, w}, {n, n, n, 6 * n, n}, {qdd, g_q, g_qd, g_tau, g_fext},
                                   {n, n, n, n, 6 * n}, 0, false, batch, check, [&](T **i, T **o, hipStream_t s) {
        return fd_vjp_batch<T>(mb, true, i[0], i[1], i[2], i[3], i[4], o[0], o[1], o[2], o[3], o[4], batch, batch, s);
    });
}

template <typename T>
int link_pose_host(const Multibody *mb, const T *q, T *pos, T *rot, int64_t batch) {
    const int64_t n = mb ? mb->model.n : 0;
    return host_call_rows<T, 1, 2>(
        mb, {q}, {n}, {pos, rot}, {3 * n, 9 * n}, 0, false, batch,
        [&] { return link_kin_args_ok<T>(mb, false, {q}, {pos, rot}); },
        [&](T **i, T **o, hipStream_t s) { return link_pose_batch<T>(mb, i[0], o[0], o[1], batch, batch, s); });
}

template <typename T>
int link_vel_host(const Multibody *mb, const T *q, const T *qd, T *vel, int64_t batch) {
    const int64_t n = mb ? mb->model.n : 0;
    return host_call_rows<T, 2, 1>(
        mb, {q, qd}, {n, n}, {vel}, {6 * n}, 0, false, batch,
        [&] { return link_kin_args_ok<T>(mb, true, {q, qd}, {vel}); },
        [&](T **i, T **o, hipStream_t s) { return link_vel_batch<T>(mb, i[0], i[1], o[0], batch, batch, s); });
}

template <typename T>
int com_host(const Multibody *mb, bool cmm, const T *q, T *out, int64_t batch) {
    const int64_t n = mb ? mb->model.n : 0;
    return host_call_rows<T, 1, 1>(
        mb, {q}, {n}, {out}, {cmm ? 6 * n : 3}, 0, false, batch,
        [&] { return centroidal_args_ok<T>(mb, cmm ? 2 : 0, {q}, {out}); },
        [&](T **i, T **o, hipStream_t s) { return com_batch<T>(mb, cmm, i[0], o[0], batch, batch, s); });
}

template <typename T>
int centroidal_host(const Multibody *mb, const T *q, const T *qd, T *com, T *hg, T *energy, int64_t batch) {
    const int64_t n = mb ? mb->model.n : 0;
    return host_call_rows<T, 2, 3>(
        mb, {q, qd}, {n, n}, {com, hg, energy}, {3, 6, 2}, 0, false, batch,
        [&] { return centroidal_args_ok<T>(mb, 1, {q, qd}, {com, hg, energy}); },
        [&](T **i, T **o, hipStream_t s) {
            return centroidal_batch<T>(mb, i[0], i[1], o[0], o[1], o[2], batch, batch, s);
        });
}

template <typename T>
int contact_wrench_host(const Multibody *mb, const T *q, const T *qd, T *fext, T *cforce, int64_t batch) {
    const int64_t n = mb ? mb->model.n : 0, np = mb ? mb->model.contacts.n_points : 0;
    return host_call_rows<T, 2, 2>(
        mb, {q, qd}, {n, n}, {fext, cforce}, {6 * n, 3 * np}, 0, false, batch,
        [&] { return contact_args_ok<T>(mb, false, {q, qd}, {fext, cforce}); },
        [&](T **i, T **o, hipStream_t s) { return contact_wrench_batch<T>(mb, i[0], i[1], o[0], o[1], batch, batch, s); });
}

// q and qd are read and written: their device copies go back to the host after the launch.
template <typename T>
int rollout_contact_host(const Multibody *mb, T *q, T *qd, const T *tau_seq, double dt, int K, T *traj, int64_t batch) {
    bool done = false;
    if (int rc = rollout_steps(mb, batch, batch, K, &done)) return rc;
    if (done) return RB_OK;
    const int64_t n = mb->model.n, kn = (int64_t)K * n;
    return host_call_rows<T, 3, 1>(
        mb, {q, qd, tau_seq}, {n, n, kn}, {traj}, {kn}, 0, false, batch,
        [&] { return contact_args_ok<T>(mb, true, {tau_seq}, {q, qd, traj}); },
        [&](T **i, T **o, hipStream_t s) {
            int rc = rollout_contact_batch<T>(mb, i[0], i[1], i[2], dt, K, o[0], batch, batch, s);
            const size_t bytes = (size_t)n * (size_t)batch * sizeof(T);
            hipError_t e = hipSuccess;
            if (rc == RB_OK) e = hipMemcpyAsync(q, i[0], bytes, hipMemcpyDeviceToHost, s);
            if (rc == RB_OK && e == hipSuccess) e = hipMemcpyAsync(qd, i[1], bytes, hipMemcpyDeviceToHost, s);
            return e == hipSuccess ? rc : hip_err(e, "hipMemcpyAsync D2H");
        });
}

template <typename T>
int rollout_vjp_host(const Multibody *mb, bool contact, const T *q, const T *qd, const T *tau_seq, double dt, int K, const T *gq,
                     const T *gqd, T *g_q0, T *g_qd0, T *g_tau, int64_t batch) {
    // the step count comes before the arrays, as in the device form
    int rc = check_batch(mb, batch, batch);
    if (rc) return rc;
    if (batch == 0) return RB_OK;
    if ((rc = vjp_steps_ok(contact, K))) return rc;
    const int64_t n = mb->model.n, kn = (int64_t)K * n;
    return host_call_rows<T, 5, 3>(
        mb, {q, qd, tau_seq, gq, gqd}, {n, n, kn, kn, kn}, {g_q0, g_qd0, g_tau}, {n, n, kn}, 2 * kn, false, batch,
        [&] { return vjp_args_ok<T>(mb, contact, {q, qd, tau_seq, gq, gqd}, {g_q0, g_qd0, g_tau}); },
        [&](T **i, T **o, hipStream_t s) {
            return rollout_vjp_batch<T>(mb, contact, i[0], i[1], i[2], dt, K, i[3], i[4], o[0], o[1], o[2], o[3], batch, batch, s);
        });
}
}  // namespace

namespace {
template <typename T>
int fill_uniform(T *x, int rows, int64_t batch, int64_t ld, const double *lo, const double *hi, uint64_t seed,
                 void *stream) {
    if (!x || !lo || !hi) return set_err(RB_ERR_NULL, "NULL argument");
    if (rows < 1 || batch < 0 || ld < batch) return set_err(RB_ERR_ARG, "bad fill shape");
    // one launch; the generator's lane index is 32-bit (b * sizeof(T) < 2^32 as the dynamics)
    if (batch > kChunk) return set_err(RB_ERR_ARG, "fill batch above 2^28 configurations not supported");
    if (batch == 0) return RB_OK;
    hipStream_t s = (hipStream_t)stream;
    std::vector<double> lohi(2 * (size_t)rows);
    for (int j = 0; j < rows; ++j) {
        lohi[2 * j] = lo[j];
        lohi[2 * j + 1] = hi[j];
    }
    double *d = nullptr;
    hipError_t e = hipMallocAsync((void **)&d, lohi.size() * sizeof(double), s);
    if (e != hipSuccess) return hip_err(e, "hipMallocAsync");
    e = hipMemcpyAsync(d, lohi.data(), lohi.size() * sizeof(double), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_err(e, "hipMemcpyAsync");
    int rc = RB_OK;
    e = rbamd::launch_fill_uniform<T>(x, rows, (uint32_t)batch, ld, d, seed, s);
    if (e != hipSuccess) rc = hip_err(e, "fill launch");
    (void)hipFreeAsync(d, s);
    // the host-side lohi vector dies here; make sure the copy has consumed it
    e = hipStreamSynchronize(s);
    if (rc == RB_OK && e != hipSuccess) rc = hip_err(e, "hipStreamSynchronize");
    return rc;
}
}  // namespace

extern "C" {

// ------------------------------------------------------------- reference ABI (6)
Multibody *multibody_new(void) {
    if (const char *path = std::getenv("RIGIDBODY_URDF")) {
        if (*path) return multibody_new_from_urdf(path);
    }
    return new_from_text(std::string(kFr3Urdf));
}

void multibody_free(Multibody *mb) { delete mb; }  // ~DeviceCache frees what it put on the devices

double *multibody_rnea(const Multibody *mb, const double *q, const double *dq, const double *ddq) {
    const size_t n = mb ? (size_t)mb->model.n : 0;
    return single_config(
        mb, {q, dq, ddq}, n, "rnea launch",
        [&](double *o) { return rbamd::host_rnea(mb->model, mb->pk64.data(), q, dq, ddq, o); },
        [&](const double *mdl, double *din, double *dout, hipStream_t s) {
            return launch_rnea_any<double>(mb, mdl, din, din + n, din + 2 * n, dout, 1, 1, s);
        });
}

double *multibody_crba(const Multibody *mb, const double *q) {
    const size_t n = mb ? (size_t)mb->model.n : 0;
    return single_config(
        mb, {q}, n * n, "crba launch", [&](double *o) { return rbamd::host_crba(mb->model, mb->pk64.data(), q, o); },
        [&](const double *mdl, double *din, double *dout, hipStream_t s) {
            return launch_crba_any<double>(mb, mdl, din, dout, 1, 1, s);
        });
}

double *multibody_fwd_kin(const Multibody *mb, const double *q) {
    return single_config(
        mb, {q}, 3, "fwd_kin launch", [&](double *o) { return rbamd::host_fwd_kin(mb->model, mb->pk64.data(), q, o); },
        [&](const double *mdl, double *din, double *dout, hipStream_t s) {
            return launch_kin_any<double>(mb, false, mdl, din, dout, 1, 1, s);
        });
}

double *multibody_jac(const Multibody *mb, const double *q) {
    const size_t n = mb ? (size_t)mb->model.n : 0;
    return single_config(
        mb, {q}, 6 * n, "jac launch", [&](double *o) { return rbamd::host_jac(mb->model, mb->pk64.data(), q, o); },
        [&](const double *mdl, double *din, double *dout, hipStream_t s) {
            return launch_kin_any<double>(mb, true, mdl, din, dout, 1, 1, s);
        });
}

// ---------------------------------------------------------------- model handling
Multibody *multibody_new_from_urdf_ex(const char *path, unsigned flags) {
    if (!path) { set_err(RB_ERR_NULL, "NULL path"); return nullptr; }
    std::ifstream f(path, std::ios::binary);
    if (!f) { set_err(RB_ERR_URDF, std::string("cannot open URDF: ") + path); return nullptr; }
    std::stringstream ss;
    ss << f.rdbuf();
    return new_from_text(ss.str(), flags);
}

Multibody *multibody_new_from_urdf_string_ex(const char *xml, size_t len, unsigned flags) {
    if (!xml) { set_err(RB_ERR_NULL, "NULL URDF string"); return nullptr; }
    return new_from_text(std::string(xml, len), flags);
}

Multibody *multibody_new_from_urdf(const char *path) { return multibody_new_from_urdf_ex(path, 0); }

Multibody *multibody_new_from_urdf_string(const char *xml, size_t len) {
    return multibody_new_from_urdf_string_ex(xml, len, 0);
}

unsigned multibody_flags(const Multibody *mb) {
    if (!mb) { set_err(RB_ERR_NULL, "NULL Multibody handle"); return 0u; }
    return mb->model.flags;
}

int64_t multibody_blob_size(const Multibody *mb) {
    if (!mb) return -set_err(RB_ERR_NULL, "NULL Multibody handle");
    return rbamd::kBlobHeader + (int64_t)mb->model.n * rbamd::kBlobPerLink + mb->model.contacts.blob_size();
}

int multibody_export_blob(const Multibody *mb, double *out, int64_t len) {
    if (!mb || !out) return set_err(RB_ERR_NULL, "NULL argument");
    std::vector<double> b = mb->model.blob();
    if (len < (int64_t)b.size()) return set_err(RB_ERR_ARG, "blob buffer too small");
    std::memcpy(out, b.data(), b.size() * sizeof(double));
    return RB_OK;
}

Multibody *multibody_new_from_blob(const double *blob, int64_t len) {
    try {
        return make(rbamd::Model::from_blob(blob, len));
    } catch (const std::exception &ex) {
        set_err(RB_ERR_ARG, ex.what());
        return nullptr;
    }
}

Multibody *multibody_with_contacts(const Multibody *mb, const rb_contact_model *cm) {
    if (!mb) { set_err(RB_ERR_NULL, "NULL Multibody handle"); return nullptr; }
    if (!cm) { set_err(RB_ERR_NULL, "NULL contact model"); return nullptr; }
    rbamd::ContactSet c;
    c.n_points = cm->n_points;
    if (c.n_points >= 1 && c.n_points <= rbamd::kContactMaxPoints)
        for (int p = 0; p < c.n_points; ++p) {
            c.link[p] = cm->link[p];
            for (int k = 0; k < 3; ++k) c.point[p][k] = cm->point[p][k];
        }
    for (int k = 0; k < 3; ++k) c.normal[k] = cm->normal[k];
    c.offset = cm->offset;
    c.stiffness = cm->stiffness;
    c.damping = cm->damping;
    c.friction = cm->friction;
    c.slip_velocity = cm->slip_velocity;
    const std::string why = c.refusal(mb->model.n);
    if (!why.empty()) { set_err(RB_ERR_ARG, why); return nullptr; }
    rbamd::Model m = mb->model;
    m.contacts = c;
    return make(std::move(m));
}

int multibody_contact_model(const Multibody *mb, rb_contact_model *out) {
    if (!mb) return -set_err(RB_ERR_NULL, "NULL Multibody handle");
    const rbamd::ContactSet &c = mb->model.contacts;
    if (out) {
        std::memset(out, 0, sizeof *out);
        out->n_points = c.n_points;
        for (int p = 0; p < c.n_points; ++p) {
            out->link[p] = c.link[p];
            for (int k = 0; k < 3; ++k) out->point[p][k] = c.point[p][k];
        }
        for (int k = 0; k < 3; ++k) out->normal[k] = c.normal[k];
        out->offset = c.offset;
        out->stiffness = c.stiffness;
        out->damping = c.damping;
        out->friction = c.friction;
        out->slip_velocity = c.slip_velocity;
    }
    return c.n_points;
}

int multibody_dof(const Multibody *mb) { return mb ? mb->model.n : -set_err(RB_ERR_NULL, "NULL Multibody handle"); }

double multibody_total_mass(const Multibody *mb) {
    if (!mb) { set_err(RB_ERR_NULL, "NULL Multibody handle"); return std::nan(""); }
    return mb->model.total_mass();
}

int multibody_limits(const Multibody *mb, double *lower, double *upper, double *velocity, double *effort) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    for (int i = 0; i < mb->model.n; ++i) {
        const rbamd::LinkModel &L = mb->model.links[i];
        if (lower) lower[i] = L.lower;
        if (upper) upper[i] = L.upper;
        if (velocity) velocity[i] = L.velocity;
        if (effort) effort[i] = L.effort;
    }
    return RB_OK;
}

int multibody_supported_dofs(int *out, int cap) { return rbamd::supported_dofs(out, cap); }

int multibody_topology(const Multibody *mb, int *parent, int *joint_type) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    for (int i = 0; i < mb->model.n; ++i) {
        if (parent) parent[i] = mb->model.links[i].parent;
        if (joint_type) joint_type[i] = mb->model.links[i].type;
    }
    return RB_OK;
}

}  // extern "C"

// C++ helpers of the kernel-inspection entry points below
namespace {
// The size of the (first) launch a call of `batch` configurations makes (chunked).
uint32_t launch_size(int64_t batch) { return batch < kChunk ? (uint32_t)batch : (uint32_t)kChunk; }

int check_kernel_query(const Multibody *mb, int kind, int64_t batch) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (kind < 0 || kind >= rbamd::kJitPublicKinds) return set_err(RB_ERR_ARG, kKindMsg);
    if (batch < 1) return set_err(RB_ERR_ARG, "batch must be positive");
    // a kind that has no kernel for this model (the derivative kinds outside their scope)
    return deriv_supported(mb, (rbamd::JitKind)kind);
}

// The hipRTC source of the kernel a launch of `batch` configurations (tiled or SoA) would run:
// compiled here (hipRTC, gfx950, no device needed) so that the occupancy-cliff rebuild of
// jit_compile shows in it -- the source of the code object a launch really loads; the generated
// source as it stands if hipRTC fails.
std::string shaped_source(const Multibody *mb, int kind, bool f64, int64_t batch, bool tiled) {
    const rbamd::JitVariant v =
        rbamd::jit_resolve(mb->model, (rbamd::JitKind)kind, f64, launch_size(batch), tiled, fast_trig());
    // the length query and the copy of multibody_jit_source_ex come in pairs: one compile for both
    thread_local std::string t_key, t_src;
    const std::string plain = rbamd::jit_source(mb->model, v, -1);
    if (plain.empty()) return plain;  // no such kernel for this model
    const std::string key = std::to_string((uintptr_t)mb) + ":" + std::to_string(rbamd::tuning_generation()) + ":" + plain;
    if (key == t_key) return t_src;
    std::vector<char> code;
    std::string err, src;
    if (!rbamd::jit_compile(mb->model, v, "gfx950", &code, &err, &src)) src = plain;
    t_key = key;
    t_src = src;
    return src;
}

// The rollout gradient's kernel has no public kind number: its two inspection entry points check
// the handle, the batch and the model's scope here.
int check_vjp_query(const Multibody *mb, bool contact, int64_t batch) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (batch < 1) return set_err(RB_ERR_ARG, "batch must be positive");
    return deriv_supported(mb, vjp_kind(contact));
}

// rc: the query's check; a kind with no kernel for this model (RB_ERR_UNSUPPORTED) has the empty source.
int source_query(const Multibody *mb, int rc, int kind, int f64, int64_t batch, int tiled, char *buf, int64_t cap) {
    if (rc && rc != RB_ERR_UNSUPPORTED) return -rc;
    const std::string src = rc ? std::string() : shaped_source(mb, kind, f64 != 0, batch, tiled != 0);
    if (buf && cap > 0) {
        const size_t n = src.size() < (size_t)(cap - 1) ? src.size() : (size_t)(cap - 1);
        std::memcpy(buf, src.data(), n);
        buf[n] = 0;
    }
    return (int)src.size();
}

int64_t compile_query(const Multibody *mb, int kind, int f64, int64_t batch, int tiled, const char *arch) {
    const rbamd::JitVariant v =
        rbamd::jit_resolve(mb->model, (rbamd::JitKind)kind, f64 != 0, launch_size(batch), tiled != 0, fast_trig());
    std::vector<char> code;
    std::string err;
    if (!rbamd::jit_compile(mb->model, v, arch ? arch : "gfx950", &code, &err)) return -set_err(RB_ERR_HIP, err);
    return (int64_t)code.size();
}

// The external-wrench kernels have no public kind number either: fd selects fd_ext (else rnea_ext).
int check_ext_query(const Multibody *mb, int64_t batch) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (batch < 1) return set_err(RB_ERR_ARG, "batch must be positive");
    return RB_OK;
}
int ext_kind(int fd) { return (int)(fd ? rbamd::JitKind::FdExt : rbamd::JitKind::RneaExt); }
// ... nor the inverse dynamics' gradient (check_ext_query's checks): ext selects the wrench form.
int rnea_vjp_kind(int ext) { return (int)(ext ? rbamd::JitKind::RneaVjpExt : rbamd::JitKind::RneaVjp); }
// ... nor the forward dynamics' gradient (check_ext_query's checks): ext selects the wrench form.
int fd_vjp_kind(int ext) { return (int)(ext ? rbamd::JitKind::FdVjpExt : rbamd::JitKind::FdVjp); }
// ... nor the link-kinematics kernels (check_ext_query's checks): vel selects link_vel (else link_pose).
int link_kin_kind(int vel) { return (int)(vel ? rbamd::JitKind::LinkVel : rbamd::JitKind::LinkPose); }

// ... nor the centroidal kernels: which = 0 com, 1 centroidal, 2 cmm; a model without mass has none
// (RB_ERR_UNSUPPORTED, the empty source).
int check_centroidal_query(const Multibody *mb, int which, int64_t batch) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (which < 0 || which > 2) return set_err(RB_ERR_ARG, "which must be 0 com, 1 centroidal or 2 cmm");
    if (batch < 1) return set_err(RB_ERR_ARG, "batch must be positive");
    return deriv_supported(mb, centroidal_kind(which));
}

// ... nor the contact kernels: rollout selects rollout_contact (else contact_wrench); a model without
// a contact set has neither (RB_ERR_UNSUPPORTED, the empty source).
int contact_kind(int rollout) {
    return (int)(rollout ? rbamd::JitKind::RolloutContact : rbamd::JitKind::ContactWrench);
}
int check_contact_query(const Multibody *mb, int rollout, int64_t batch) {
    if (int rc = check_ext_query(mb, batch)) return rc;
    return deriv_supported(mb, (rbamd::JitKind)contact_kind(rollout));
}

void note_jit_errors(const Multibody *mb) {
    for (std::string &err : mb->cache.jit_errors()) g_last_error = std::move(err);
}
}  // namespace

extern "C" {

int multibody_kernel_path_ex(const Multibody *mb, int kind, int f64, int64_t batch, int tiled) {
    if (int rc = check_kernel_query(mb, kind, batch)) return -rc;
    if (kernel_for(mb, (rbamd::JitKind)kind, f64 != 0, launch_size(batch), tiled != 0)) return 1;
    if (rbamd::jit_enabled() && !((kind == 4 || kind == 5) && kin_precompiled(mb))) note_jit_errors(mb);
    return 0;
}

int multibody_kernel_form_ex(const Multibody *mb, int kind, int f64, int64_t batch, int tiled) {
    if (int rc = check_kernel_query(mb, kind, batch)) return -rc;
    const rbamd::JitKernel *jk = kernel_for(mb, (rbamd::JitKind)kind, f64 != 0, launch_size(batch), tiled != 0);
    return jk ? jk->variant.pack : 0;
}

int multibody_kernel_path(const Multibody *mb, int kind, int f64) {
    return multibody_kernel_path_ex(mb, kind, f64, int64_t(1) << 20, 0);
}

int multibody_rnea_kernel_path(const Multibody *mb, int f64) { return multibody_kernel_path(mb, 0, f64); }

int multibody_single_config_path(const Multibody *mb) {
    if (!mb) return -set_err(RB_ERR_NULL, "NULL Multibody handle");
    return (rbamd::tuning().single_gpu == 0 && rbamd::host_eval_supported(mb->model)) ? 0 : 1;
}

int multibody_jit_source(const Multibody *mb, int kind, int f64, char *buf, int64_t cap) {
    return multibody_jit_source_ex(mb, kind, f64, int64_t(1) << 20, 0, buf, cap);
}

int multibody_jit_source_ex(const Multibody *mb, int kind, int f64, int64_t batch, int tiled, char *buf, int64_t cap) {
    return source_query(mb, check_kernel_query(mb, kind, batch), kind, f64, batch, tiled, buf, cap);
}

int multibody_rollout_vjp_jit_source(const Multibody *mb, int f64, int64_t batch, char *buf, int64_t cap) {
    return source_query(mb, check_vjp_query(mb, false, batch), (int)vjp_kind(false), f64, batch, 0, buf, cap);
}

int multibody_contact_vjp_jit_source(const Multibody *mb, int f64, int64_t batch, char *buf, int64_t cap) {
    return source_query(mb, check_vjp_query(mb, true, batch), (int)vjp_kind(true), f64, batch, 0, buf, cap);
}

int64_t multibody_jit_compile(const Multibody *mb, int kind, int f64, const char *arch) {
    return multibody_jit_compile_ex(mb, kind, f64, int64_t(1) << 20, 0, arch);
}

int64_t multibody_jit_compile_ex(const Multibody *mb, int kind, int f64, int64_t batch, int tiled, const char *arch) {
    if (int rc = check_kernel_query(mb, kind, batch)) return -rc;
    return compile_query(mb, kind, f64, batch, tiled, arch);
}

int64_t multibody_rollout_vjp_jit_compile(const Multibody *mb, int f64, int64_t batch, const char *arch) {
    if (int rc = check_vjp_query(mb, false, batch)) return -rc;
    return compile_query(mb, (int)vjp_kind(false), f64, batch, 0, arch);
}

int64_t multibody_contact_vjp_jit_compile(const Multibody *mb, int f64, int64_t batch, const char *arch) {
    if (int rc = check_vjp_query(mb, true, batch)) return -rc;
    return compile_query(mb, (int)vjp_kind(true), f64, batch, 0, arch);
}

int multibody_ext_jit_source(const Multibody *mb, int fd, int f64, int64_t batch, char *buf, int64_t cap) {
    return source_query(mb, check_ext_query(mb, batch), ext_kind(fd), f64, batch, 0, buf, cap);
}

int64_t multibody_ext_jit_compile(const Multibody *mb, int fd, int f64, int64_t batch, const char *arch) {
    if (int rc = check_ext_query(mb, batch)) return -rc;
    return compile_query(mb, ext_kind(fd), f64, batch, 0, arch);
}

int multibody_rnea_vjp_jit_source(const Multibody *mb, int ext, int f64, int64_t batch, char *buf, int64_t cap) {
    return source_query(mb, check_ext_query(mb, batch), rnea_vjp_kind(ext), f64, batch, 0, buf, cap);
}

int64_t multibody_rnea_vjp_jit_compile(const Multibody *mb, int ext, int f64, int64_t batch, const char *arch) {
    if (int rc = check_ext_query(mb, batch)) return -rc;
    return compile_query(mb, rnea_vjp_kind(ext), f64, batch, 0, arch);
}

int multibody_fd_vjp_jit_source(const Multibody *mb, int ext, int f64, int64_t batch, char *buf, int64_t cap) {
    return source_query(mb, check_ext_query(mb, batch), fd_vjp_kind(ext), f64, batch, 0, buf, cap);
}

int64_t multibody_fd_vjp_jit_compile(const Multibody *mb, int ext, int f64, int64_t batch, const char *arch) {
    if (int rc = check_ext_query(mb, batch)) return -rc;
    return compile_query(mb, fd_vjp_kind(ext), f64, batch, 0, arch);
}

int multibody_link_kin_jit_source(const Multibody *mb, int vel, int f64, int64_t batch, char *buf, int64_t cap) {
    return source_query(mb, check_ext_query(mb, batch), link_kin_kind(vel), f64, batch, 0, buf, cap);
}

int64_t multibody_link_kin_jit_compile(const Multibody *mb, int vel, int f64, int64_t batch, const char *arch) {
    if (int rc = check_ext_query(mb, batch)) return -rc;
    return compile_query(mb, link_kin_kind(vel), f64, batch, 0, arch);
}

int multibody_centroidal_jit_source(const Multibody *mb, int which, int f64, int64_t batch, char *buf, int64_t cap) {
    return source_query(mb, check_centroidal_query(mb, which, batch), (int)centroidal_kind(which), f64, batch, 0, buf, cap);
}

int64_t multibody_centroidal_jit_compile(const Multibody *mb, int which, int f64, int64_t batch, const char *arch) {
    if (int rc = check_centroidal_query(mb, which, batch)) return -rc;
    return compile_query(mb, (int)centroidal_kind(which), f64, batch, 0, arch);
}

int multibody_contact_jit_source(const Multibody *mb, int rollout, int f64, int64_t batch, char *buf, int64_t cap) {
    return source_query(mb, check_contact_query(mb, rollout, batch), contact_kind(rollout), f64, batch, 0, buf, cap);
}

int64_t multibody_contact_jit_compile(const Multibody *mb, int rollout, int f64, int64_t batch, const char *arch) {
    if (int rc = check_contact_query(mb, rollout, batch)) return -rc;
    return compile_query(mb, contact_kind(rollout), f64, batch, 0, arch);
}

int multibody_upload(const Multibody *mb) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    const float *a = nullptr;
    const double *b = nullptr;
    int rc = device_consts<float>(mb, &a);
    if (rc) return rc;
    return device_consts<double>(mb, &b);
}

void multibody_result_free(double *p) { std::free(p); }
const char *rb_last_error(void) { return g_last_error.c_str(); }
const char *rb_version(void) { return RB_VERSION; }

}  // extern "C"

namespace {

template <typename T>
int convert_tiled(const T *src, T *dst, int64_t ld, int rows, int64_t batch, void *stream, bool to) {
    if (!src || !dst) return set_err(RB_ERR_NULL, "NULL array");
    if (rows < 0 || batch < 0 || ld < batch) return set_err(RB_ERR_ARG, "bad layout conversion shape");
    return chunked<T>(batch, [&](int64_t b0, uint32_t nb) {
        hipError_t e = to ? rbamd::launch_to_tiled<T>(src + b0, ld, dst + b0 * rows, rows, nb, (hipStream_t)stream)
                          : rbamd::launch_from_tiled<T>(src + b0 * rows, dst + b0, ld, rows, nb, (hipStream_t)stream);
        return e == hipSuccess ? RB_OK : hip_err(e, "layout conversion");
    });
}

}  // namespace

extern "C" {

int rb_to_tiled_f32(const float *src, int64_t ld, float *dst, int rows, int64_t batch, void *stream) {
    return convert_tiled<float>(src, dst, ld, rows, batch, stream, true);
}
int rb_to_tiled_f64(const double *src, int64_t ld, double *dst, int rows, int64_t batch, void *stream) {
    return convert_tiled<double>(src, dst, ld, rows, batch, stream, true);
}
int rb_from_tiled_f32(const float *src, float *dst, int64_t ld, int rows, int64_t batch, void *stream) {
    return convert_tiled<float>(src, dst, ld, rows, batch, stream, false);
}
int rb_from_tiled_f64(const double *src, double *dst, int64_t ld, int rows, int64_t batch, void *stream) {
    return convert_tiled<double>(src, dst, ld, rows, batch, stream, false);
}

int rb_set_tuning(const char *key, int value) {
    if (!key) return set_err(RB_ERR_NULL, "NULL key");
    switch (rbamd::tuning_set(key, value)) {
        case 0: return RB_OK;
        case 2: return set_err(RB_ERR_ARG, std::string("experimental tuning key (set RB_EXPERIMENTAL=1): ") + key);
        default: return set_err(RB_ERR_ARG, std::string("unknown tuning key: ") + key);
    }
}

// ------------------------------------------------------------- batched (device)
int multibody_rnea_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                             float *tau, int64_t batch, int64_t ld, void *stream) {
    return rnea_batch<float>(mb, q, qd, qdd, tau, batch, ld, stream);
}
int multibody_rnea_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                             double *tau, int64_t batch, int64_t ld, void *stream) {
    return rnea_batch<double>(mb, q, qd, qdd, tau, batch, ld, stream);
}
int multibody_fd_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *tau,
                           float *qdd, int64_t batch, int64_t ld, void *stream) {
    return fd_batch<float>(mb, q, qd, tau, qdd, batch, ld, stream);
}
int multibody_fd_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                           double *qdd, int64_t batch, int64_t ld, void *stream) {
    return fd_batch<double>(mb, q, qd, tau, qdd, batch, ld, stream);
}
int multibody_rnea_batch_tiled_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                   float *tau, int64_t batch, void *stream) {
    return rnea_batch<float>(mb, q, qd, qdd, tau, batch, 256, stream, true);
}
int multibody_rnea_batch_tiled_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                   double *tau, int64_t batch, void *stream) {
    return rnea_batch<double>(mb, q, qd, qdd, tau, batch, 256, stream, true);
}
int multibody_fd_batch_tiled_f32(const Multibody *mb, const float *q, const float *qd, const float *tau,
                                 float *qdd, int64_t batch, void *stream) {
    return fd_batch<float>(mb, q, qd, tau, qdd, batch, 256, stream, true);
}
int multibody_fd_batch_tiled_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                                 double *qdd, int64_t batch, void *stream) {
    return fd_batch<double>(mb, q, qd, tau, qdd, batch, 256, stream, true);
}
int multibody_rnea_fd_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                const float *tau_in, float *tau, float *qdd_out, int64_t batch, int64_t ld,
                                void *stream) {
    return idfd_batch<float>(mb, q, qd, qdd, tau_in, tau, qdd_out, batch, ld, stream);
}
int multibody_rnea_fd_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                const double *tau_in, double *tau, double *qdd_out, int64_t batch, int64_t ld,
                                void *stream) {
    return idfd_batch<double>(mb, q, qd, qdd, tau_in, tau, qdd_out, batch, ld, stream);
}
int multibody_rnea_fd_batch_tiled_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                      const float *tau_in, float *tau, float *qdd_out, int64_t batch, void *stream) {
    return idfd_batch<float>(mb, q, qd, qdd, tau_in, tau, qdd_out, batch, 256, stream, true);
}
int multibody_rnea_fd_batch_tiled_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                      const double *tau_in, double *tau, double *qdd_out, int64_t batch,
                                      void *stream) {
    return idfd_batch<double>(mb, q, qd, qdd, tau_in, tau, qdd_out, batch, 256, stream, true);
}
int multibody_rollout_batch_f32(const Multibody *mb, float *q, float *qd, const float *tau_seq, double dt, int K,
                                 float *traj, int64_t batch, int64_t ld, void *stream) {
    return rollout_batch<float>(mb, q, qd, tau_seq, dt, K, traj, batch, ld, stream);
}
int multibody_rollout_batch_f64(const Multibody *mb, double *q, double *qd, const double *tau_seq, double dt, int K,
                                 double *traj, int64_t batch, int64_t ld, void *stream) {
    return rollout_batch<double>(mb, q, qd, tau_seq, dt, K, traj, batch, ld, stream);
}
int multibody_crba_batch_f32(const Multibody *mb, const float *q, float *H, int64_t batch, int64_t ld,
                             void *stream) {
    return crba_batch<float>(mb, q, H, batch, ld, stream);
}
int multibody_crba_batch_f64(const Multibody *mb, const double *q, double *H, int64_t batch, int64_t ld,
                             void *stream) {
    return crba_batch<double>(mb, q, H, batch, ld, stream);
}

int multibody_crba_batch_tiled_f32(const Multibody *mb, const float *q, float *H, int64_t batch, void *stream) {
    return crba_batch<float>(mb, q, H, batch, 256, stream, true);
}
int multibody_crba_batch_tiled_f64(const Multibody *mb, const double *q, double *H, int64_t batch, void *stream) {
    return crba_batch<double>(mb, q, H, batch, 256, stream, true);
}
int multibody_fwd_kin_batch_tiled_f32(const Multibody *mb, const float *q, float *pos, int64_t batch, void *stream) {
    return kin_batch<float>(mb, false, q, pos, batch, 256, stream, true);
}
int multibody_fwd_kin_batch_tiled_f64(const Multibody *mb, const double *q, double *pos, int64_t batch,
                                      void *stream) {
    return kin_batch<double>(mb, false, q, pos, batch, 256, stream, true);
}
int multibody_jac_batch_tiled_f32(const Multibody *mb, const float *q, float *J, int64_t batch, void *stream) {
    return kin_batch<float>(mb, true, q, J, batch, 256, stream, true);
}
int multibody_jac_batch_tiled_f64(const Multibody *mb, const double *q, double *J, int64_t batch, void *stream) {
    return kin_batch<double>(mb, true, q, J, batch, 256, stream, true);
}

int multibody_fwd_kin_batch_f64(const Multibody *mb, const double *q, double *pos, int64_t batch,
                                int64_t ld, void *stream) {
    return kin_batch<double>(mb, false, q, pos, batch, ld, stream);
}
int multibody_jac_batch_f64(const Multibody *mb, const double *q, double *J, int64_t batch, int64_t ld,
                            void *stream) {
    return kin_batch<double>(mb, true, q, J, batch, ld, stream);
}
int multibody_fwd_kin_batch_f32(const Multibody *mb, const float *q, float *pos, int64_t batch, int64_t ld,
                                void *stream) {
    return kin_batch<float>(mb, false, q, pos, batch, ld, stream);
}
int multibody_jac_batch_f32(const Multibody *mb, const float *q, float *J, int64_t batch, int64_t ld,
                            void *stream) {
    return kin_batch<float>(mb, true, q, J, batch, ld, stream);
}

// ------------------------------------------------------------- analytical derivatives
int multibody_rnea_deriv_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                   float *dtau_dq, float *dtau_dqd, int64_t batch, int64_t ld, void *stream) {
    return rnea_deriv_batch<float>(mb, q, qd, qdd, dtau_dq, dtau_dqd, batch, ld, stream);
}
int multibody_rnea_deriv_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                   double *dtau_dq, double *dtau_dqd, int64_t batch, int64_t ld, void *stream) {
    return rnea_deriv_batch<double>(mb, q, qd, qdd, dtau_dq, dtau_dqd, batch, ld, stream);
}
int multibody_fd_deriv_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *tau, float *qdd_out,
                                 float *dqdd_dq, float *dqdd_dqd, float *dqdd_dtau, int64_t batch, int64_t ld,
                                 void *stream) {
    return fd_deriv_batch<float>(mb, q, qd, tau, qdd_out, dqdd_dq, dqdd_dqd, dqdd_dtau, batch, ld, stream);
}
int multibody_fd_deriv_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                                 double *qdd_out, double *dqdd_dq, double *dqdd_dqd, double *dqdd_dtau, int64_t batch,
                                 int64_t ld, void *stream) {
    return fd_deriv_batch<double>(mb, q, qd, tau, qdd_out, dqdd_dq, dqdd_dqd, dqdd_dtau, batch, ld, stream);
}
int multibody_rnea_deriv_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                        float *dtau_dq, float *dtau_dqd, int64_t batch) {
    return rnea_deriv_host<float>(mb, q, qd, qdd, dtau_dq, dtau_dqd, batch);
}
int multibody_rnea_deriv_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                        double *dtau_dq, double *dtau_dqd, int64_t batch) {
    return rnea_deriv_host<double>(mb, q, qd, qdd, dtau_dq, dtau_dqd, batch);
}
int multibody_fd_deriv_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *tau,
                                      float *qdd_out, float *dqdd_dq, float *dqdd_dqd, float *dqdd_dtau,
                                      int64_t batch) {
    return fd_deriv_host<float>(mb, q, qd, tau, qdd_out, dqdd_dq, dqdd_dqd, dqdd_dtau, batch);
}
int multibody_fd_deriv_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                                      double *qdd_out, double *dqdd_dq, double *dqdd_dqd, double *dqdd_dtau,
                                      int64_t batch) {
    return fd_deriv_host<double>(mb, q, qd, tau, qdd_out, dqdd_dq, dqdd_dqd, dqdd_dtau, batch);
}

// ------------------------------------------------------------- gradient of the rollout
int multibody_rollout_vjp_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *tau_seq, double dt,
                                    int K, const float *gq, const float *gqd, float *g_q0, float *g_qd0, float *g_tau,
                                    float *work, int64_t batch, int64_t ld, void *stream) {
    return rollout_vjp_batch<float>(mb, false, q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau, work, batch, ld, stream);
}
int multibody_rollout_vjp_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *tau_seq,
                                    double dt, int K, const double *gq, const double *gqd, double *g_q0, double *g_qd0,
                                    double *g_tau, double *work, int64_t batch, int64_t ld, void *stream) {
    return rollout_vjp_batch<double>(mb, false, q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau, work, batch, ld, stream);
}
int multibody_rollout_vjp_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *tau_seq,
                                         double dt, int K, const float *gq, const float *gqd, float *g_q0, float *g_qd0,
                                         float *g_tau, int64_t batch) {
    return rollout_vjp_host<float>(mb, false, q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau, batch);
}
int multibody_rollout_vjp_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *tau_seq,
                                         double dt, int K, const double *gq, const double *gqd, double *g_q0,
                                         double *g_qd0, double *g_tau, int64_t batch) {
    return rollout_vjp_host<double>(mb, false, q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau, batch);
}

int multibody_rollout_vjp(const Multibody *mb, const double *q, const double *qd, const double *tau_seq, double dt, int K,
                          const double *gq, const double *gqd, double *g_q0, double *g_qd0, double *g_tau) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (int rc = vjp_steps_ok(false, K)) return rc;
    if (int rc = vjp_args_ok<double>(mb, false, {q, qd, tau_seq, gq, gqd}, {g_q0, g_qd0, g_tau})) return rc;
    if (!rbamd::host_rollout_vjp(mb->model, mb->pk64.data(), q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau))
        return set_err(RB_ERR_UNSUPPORTED, "rollout_vjp: the single-configuration form runs on the host and needs an "
                                           "FMA3 / AVX2 CPU");
    return RB_OK;
}

// ------------------------------------------------------------- gradient of the contact rollout
int multibody_rollout_contact_vjp_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *tau_seq, double dt,
                                    int K, const float *gq, const float *gqd, float *g_q0, float *g_qd0, float *g_tau,
                                    float *work, int64_t batch, int64_t ld, void *stream) {
    return rollout_vjp_batch<float>(mb, true, q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau, work, batch, ld, stream);
}
int multibody_rollout_contact_vjp_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *tau_seq,
                                    double dt, int K, const double *gq, const double *gqd, double *g_q0, double *g_qd0,
                                    double *g_tau, double *work, int64_t batch, int64_t ld, void *stream) {
    return rollout_vjp_batch<double>(mb, true, q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau, work, batch, ld, stream);
}
int multibody_rollout_contact_vjp_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *tau_seq,
                                         double dt, int K, const float *gq, const float *gqd, float *g_q0, float *g_qd0,
                                         float *g_tau, int64_t batch) {
    return rollout_vjp_host<float>(mb, true, q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau, batch);
}
int multibody_rollout_contact_vjp_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *tau_seq,
                                         double dt, int K, const double *gq, const double *gqd, double *g_q0,
                                         double *g_qd0, double *g_tau, int64_t batch) {
    return rollout_vjp_host<double>(mb, true, q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau, batch);
}

int multibody_rollout_contact_vjp(const Multibody *mb, const double *q, const double *qd, const double *tau_seq, double dt, int K,
                          const double *gq, const double *gqd, double *g_q0, double *g_qd0, double *g_tau) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (int rc = vjp_steps_ok(true, K)) return rc;
    if (int rc = vjp_args_ok<double>(mb, true, {q, qd, tau_seq, gq, gqd}, {g_q0, g_qd0, g_tau})) return rc;
    if (!rbamd::host_rollout_contact_vjp(mb->model, mb->pk64.data(), mb->ra64.data(), q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau))
        return set_err(RB_ERR_UNSUPPORTED, "rollout_contact_vjp: the single-configuration form runs on the host and needs an "
                                           "FMA3 / AVX2 CPU");
    return RB_OK;
}

// Single configuration, fp64, on the calling thread: the lane body compiled for the host
// (host_eval.cpp); no GPU involved.
int multibody_rnea_deriv(const Multibody *mb, const double *q, const double *qd, const double *qdd, double *dtau_dq,
                         double *dtau_dqd) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (int rc = deriv_args_ok<double>(mb, rbamd::JitKind::RneaDeriv, "rnea_deriv", {q, qd, qdd}, {dtau_dq, dtau_dqd}))
        return rc;
    if (!rbamd::host_rnea_deriv(mb->model, mb->pk64.data(), q, qd, qdd, dtau_dq, dtau_dqd))
        return set_err(RB_ERR_UNSUPPORTED, "rnea_deriv: the single-configuration form runs on the host and needs an "
                                           "FMA3 / AVX2 CPU");
    return RB_OK;
}

int multibody_fd_deriv(const Multibody *mb, const double *q, const double *qd, const double *tau, double *qdd,
                       double *dqdd_dq, double *dqdd_dqd, double *dqdd_dtau) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (int rc = deriv_args_ok<double>(mb, rbamd::JitKind::FdDeriv, "fd_deriv", {q, qd, tau},
                                       {qdd, dqdd_dq, dqdd_dqd, dqdd_dtau}))
        return rc;
    if (!rbamd::host_fd_deriv(mb->model, mb->pk64.data(), q, qd, tau, qdd, dqdd_dq, dqdd_dqd, dqdd_dtau))
        return set_err(RB_ERR_UNSUPPORTED, "fd_deriv: the single-configuration form runs on the host and needs an "
                                           "FMA3 / AVX2 CPU");
    return RB_OK;
}

// ------------------------------------------------------------- external link wrenches
int multibody_rnea_ext_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                 const float *fext, float *tau, int64_t batch, int64_t ld, void *stream) {
    return ext_batch<float>(mb, false, q, qd, qdd, fext, tau, batch, ld, stream);
}
int multibody_rnea_ext_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                 const double *fext, double *tau, int64_t batch, int64_t ld, void *stream) {
    return ext_batch<double>(mb, false, q, qd, qdd, fext, tau, batch, ld, stream);
}
int multibody_fd_ext_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *tau,
                               const float *fext, float *qdd, int64_t batch, int64_t ld, void *stream) {
    return ext_batch<float>(mb, true, q, qd, tau, fext, qdd, batch, ld, stream);
}
int multibody_fd_ext_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                               const double *fext, double *qdd, int64_t batch, int64_t ld, void *stream) {
    return ext_batch<double>(mb, true, q, qd, tau, fext, qdd, batch, ld, stream);
}
int multibody_rnea_ext_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                      const float *fext, float *tau, int64_t batch) {
    return ext_host<float>(mb, false, q, qd, qdd, fext, tau, batch);
}
int multibody_rnea_ext_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                      const double *fext, double *tau, int64_t batch) {
    return ext_host<double>(mb, false, q, qd, qdd, fext, tau, batch);
}
int multibody_fd_ext_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *tau,
                                    const float *fext, float *qdd, int64_t batch) {
    return ext_host<float>(mb, true, q, qd, tau, fext, qdd, batch);
}
int multibody_fd_ext_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                                    const double *fext, double *qdd, int64_t batch) {
    return ext_host<double>(mb, true, q, qd, tau, fext, qdd, batch);
}

// Single configuration, fp64, on the calling thread (host_eval.cpp): serial revolute chains of a
// multibody_supported_dofs length.
static int ext_single(const Multibody *mb, bool fd, const double *q, const double *qd, const double *third,
                      const double *fext, double *out) {
    const char *op = fd ? "fd_ext" : "rnea_ext";
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (int rc = ext_args_ok<double>(op, {q, qd, third, fext}, out)) return rc;
    if (!mb->model.serial_revolute())
        return set_err(RB_ERR_UNSUPPORTED, std::string(op) + ": the single-configuration form evaluates serial revolute "
                                           "chains only (kinematic trees, prismatic joints and a floating base take "
                                           "the batched entry points)");
    const bool ok = fd ? rbamd::host_fd_ext(mb->model, mb->pk64.data(), mb->ra64.data(), q, qd, third, fext, out)
                       : rbamd::host_rnea_ext(mb->model, mb->pk64.data(), mb->ra64.data(), q, qd, third, fext, out);
    if (!ok)
        return set_err(RB_ERR_UNSUPPORTED, std::string(op) + ": the single-configuration form runs on the host and "
                                           "needs an FMA3 / AVX2 CPU");
    return RB_OK;
}
int multibody_rnea_ext(const Multibody *mb, const double *q, const double *qd, const double *qdd, const double *fext,
                       double *tau) {
    return ext_single(mb, false, q, qd, qdd, fext, tau);
}
int multibody_fd_ext(const Multibody *mb, const double *q, const double *qd, const double *tau, const double *fext,
                     double *qdd) {
    return ext_single(mb, true, q, qd, tau, fext, qdd);
}

// ------------------------------------------- reverse-mode gradient of the inverse dynamics
int multibody_rnea_vjp_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                 const float *fext, const float *w, float *g_q, float *g_qd, float *g_qdd,
                                 float *g_fext, int64_t batch, int64_t ld, void *stream) {
    return rnea_vjp_batch<float>(mb, true, q, qd, qdd, fext, w, g_q, g_qd, g_qdd, g_fext, batch, ld, stream);
}
int multibody_rnea_vjp_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                      const float *fext, const float *w, float *g_q, float *g_qd, float *g_qdd,
                                      float *g_fext, int64_t batch) {
    return rnea_vjp_host<float>(mb, true, q, qd, qdd, fext, w, g_q, g_qd, g_qdd, g_fext, batch);
}
int multibody_rnea_vjp_plain_batch_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                       const float *w, float *g_q, float *g_qd, float *g_qdd, int64_t batch,
                                       int64_t ld, void *stream) {
    return rnea_vjp_batch<float>(mb, false, q, qd, qdd, nullptr, w, g_q, g_qd, g_qdd, nullptr, batch, ld, stream);
}
int multibody_rnea_vjp_plain_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                            const float *w, float *g_q, float *g_qd, float *g_qdd, int64_t batch) {
    return rnea_vjp_host<float>(mb, false, q, qd, qdd, nullptr, w, g_q, g_qd, g_qdd, nullptr, batch);
}
int multibody_rnea_vjp_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                 const double *fext, const double *w, double *g_q, double *g_qd, double *g_qdd,
                                 double *g_fext, int64_t batch, int64_t ld, void *stream) {
    return rnea_vjp_batch<double>(mb, true, q, qd, qdd, fext, w, g_q, g_qd, g_qdd, g_fext, batch, ld, stream);
}
int multibody_rnea_vjp_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                      const double *fext, const double *w, double *g_q, double *g_qd, double *g_qdd,
                                      double *g_fext, int64_t batch) {
    return rnea_vjp_host<double>(mb, true, q, qd, qdd, fext, w, g_q, g_qd, g_qdd, g_fext, batch);
}
int multibody_rnea_vjp_plain_batch_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                       const double *w, double *g_q, double *g_qd, double *g_qdd, int64_t batch,
                                       int64_t ld, void *stream) {
    return rnea_vjp_batch<double>(mb, false, q, qd, qdd, nullptr, w, g_q, g_qd, g_qdd, nullptr, batch, ld, stream);
}
int multibody_rnea_vjp_plain_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                            const double *w, double *g_q, double *g_qd, double *g_qdd,
                                            int64_t batch) {
    return rnea_vjp_host<double>(mb, false, q, qd, qdd, nullptr, w, g_q, g_qd, g_qdd, nullptr, batch);
}

// Single configuration, fp64, on the calling thread (host_eval.cpp): multibody_rnea_ext's scope.
int multibody_rnea_vjp(const Multibody *mb, const double *q, const double *qd, const double *qdd, const double *fext,
                       const double *w, double *g_q, double *g_qd, double *g_qdd, double *g_fext) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (int rc = rnea_vjp_args_ok<double>(true, true, q, qd, qdd, fext, w, g_q, g_qd, g_qdd, g_fext)) return rc;
    if (!mb->model.serial_revolute())
        return set_err(RB_ERR_UNSUPPORTED, "rnea_vjp: the single-configuration form evaluates serial revolute chains only "
                                           "(kinematic trees, prismatic joints and a floating base take the batched "
                                           "entry points)");
    if (!rbamd::host_rnea_vjp(mb->model, mb->pk64.data(), mb->ra64.data(), q, qd, qdd, fext, w, g_q, g_qd, g_qdd, g_fext))
        return set_err(RB_ERR_UNSUPPORTED, "rnea_vjp: the single-configuration form runs on the host and needs an FMA3 / "
                                           "AVX2 CPU");
    return RB_OK;
}

// ------------------------------------------- reverse-mode gradient of the forward dynamics
#define RB_FD_VJP_ENTRY(T, sfx)                                                                                          \
    int multibody_fd_vjp_batch_##sfx(const Multibody *mb, const T *q, const T *qd, const T *tau, const T *fext,          \
                                     const T *w, T *qdd, T *g_q, T *g_qd, T *g_tau, T *g_fext, int64_t batch,            \
                                     int64_t ld, void *stream) {                                                         \
        return fd_vjp_batch<T>(mb, true, q, qd, tau, fext, w, qdd, g_q, g_qd, g_tau, g_fext, batch, ld, stream);         \
    }                                                                                                                    \
    int multibody_fd_vjp_batch_host_##sfx(const Multibody *mb, const T *q, const T *qd, const T *tau, const T *fext,     \
                                          const T *w, T *qdd, T *g_q, T *g_qd, T *g_tau, T *g_fext, int64_t batch) {     \
        return fd_vjp_host<T>(mb, true, q, qd, tau, fext, w, qdd, g_q, g_qd, g_tau, g_fext, batch);                      \
    }                                                                                                                    \
    int multibody_fd_vjp_plain_batch_##sfx(const Multibody *mb, const T *q, const T *qd, const T *tau, const T *w,       \
                                           T *qdd, T *g_q, T *g_qd, T *g_tau, int64_t batch, int64_t ld,                 \
                                           void *stream) {                                                               \
        return fd_vjp_batch<T>(mb, false, q, qd, tau, nullptr, w, qdd, g_q, g_qd, g_tau, nullptr, batch, ld, stream);    \
    }                                                                                                                    \
    int multibody_fd_vjp_plain_batch_host_##sfx(const Multibody *mb, const T *q, const T *qd, const T *tau, const T *w,  \
                                                T *qdd, T *g_q, T *g_qd, T *g_tau, int64_t batch) {                      \
        return fd_vjp_host<T>(mb, false, q, qd, tau, nullptr, w, qdd, g_q, g_qd, g_tau, nullptr, batch);                 \
    }
RB_FD_VJP_ENTRY(float, f32)
RB_FD_VJP_ENTRY(double, f64)
#undef RB_FD_VJP_ENTRY

// Single configuration, fp64, on the calling thread (host_eval.cpp): multibody_rnea_vjp's scope.
int multibody_fd_vjp(const Multibody *mb, const double *q, const double *qd, const double *tau, const double *fext,
                     const double *w, double *qdd, double *g_q, double *g_qd, double *g_tau, double *g_fext) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (int rc = fd_vjp_args_ok<double>(true, true, q, qd, tau, fext, w, qdd, g_q, g_qd, g_tau, g_fext)) return rc;
    if (!mb->model.serial_revolute())
        return set_err(RB_ERR_UNSUPPORTED, "fd_vjp: the single-configuration form evaluates serial revolute chains only "
                                           "(kinematic trees, prismatic joints and a floating base take the batched "
                                           "entry points)");
    if (!rbamd::host_fd_vjp(mb->model, mb->pk64.data(), mb->ra64.data(), q, qd, tau, fext, w, qdd, g_q, g_qd, g_tau, g_fext))
        return set_err(RB_ERR_UNSUPPORTED, "fd_vjp: the single-configuration form runs on the host and needs an FMA3 / "
                                           "AVX2 CPU");
    return RB_OK;
}

// ------------------------------------------------------------- kinematics of every link
int multibody_link_pose_batch_f32(const Multibody *mb, const float *q, float *pos, float *rot, int64_t batch,
                                  int64_t ld, void *stream) {
    return link_pose_batch<float>(mb, q, pos, rot, batch, ld, stream);
}
int multibody_link_pose_batch_f64(const Multibody *mb, const double *q, double *pos, double *rot, int64_t batch,
                                  int64_t ld, void *stream) {
    return link_pose_batch<double>(mb, q, pos, rot, batch, ld, stream);
}
int multibody_link_vel_batch_f32(const Multibody *mb, const float *q, const float *qd, float *vel, int64_t batch,
                                 int64_t ld, void *stream) {
    return link_vel_batch<float>(mb, q, qd, vel, batch, ld, stream);
}
int multibody_link_vel_batch_f64(const Multibody *mb, const double *q, const double *qd, double *vel, int64_t batch,
                                 int64_t ld, void *stream) {
    return link_vel_batch<double>(mb, q, qd, vel, batch, ld, stream);
}
int multibody_link_pose_batch_host_f32(const Multibody *mb, const float *q, float *pos, float *rot, int64_t batch) {
    return link_pose_host<float>(mb, q, pos, rot, batch);
}
int multibody_link_pose_batch_host_f64(const Multibody *mb, const double *q, double *pos, double *rot, int64_t batch) {
    return link_pose_host<double>(mb, q, pos, rot, batch);
}
int multibody_link_vel_batch_host_f32(const Multibody *mb, const float *q, const float *qd, float *vel,
                                      int64_t batch) {
    return link_vel_host<float>(mb, q, qd, vel, batch);
}
int multibody_link_vel_batch_host_f64(const Multibody *mb, const double *q, const double *qd, double *vel,
                                      int64_t batch) {
    return link_vel_host<double>(mb, q, qd, vel, batch);
}

// Single configuration, fp64, on the calling thread (host_eval.cpp): serial revolute chains of a
// multibody_supported_dofs length.
static int link_kin_single(const Multibody *mb, bool vel, const double *q, const double *qd, double *out0,
                           double *out1) {
    const char *op = vel ? "link_vel" : "link_pose";
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (int rc = vel ? link_kin_args_ok<double>(mb, true, {q, qd}, {out0})
                     : link_kin_args_ok<double>(mb, false, {q}, {out0, out1}))
        return rc;
    if (!mb->model.serial_revolute())
        return set_err(RB_ERR_UNSUPPORTED, std::string(op) + ": the single-configuration form evaluates serial revolute "
                                           "chains only (kinematic trees, prismatic joints and a floating base take "
                                           "the batched entry points)");
    const bool ok = vel ? rbamd::host_link_vel(mb->model, mb->pk64.data(), mb->ra64.data(), q, qd, out0)
                        : rbamd::host_link_pose(mb->model, mb->pk64.data(), mb->ra64.data(), q, out0, out1);
    if (!ok)
        return set_err(RB_ERR_UNSUPPORTED, std::string(op) + ": the single-configuration form runs on the host and "
                                           "needs an FMA3 / AVX2 CPU");
    return RB_OK;
}
int multibody_link_pose(const Multibody *mb, const double *q, double *pos, double *rot) {
    return link_kin_single(mb, false, q, nullptr, pos, rot);
}
int multibody_link_vel(const Multibody *mb, const double *q, const double *qd, double *vel) {
    return link_kin_single(mb, true, q, qd, vel, nullptr);
}

// ------------------------------------------------- centre of mass, centroidal momentum, energy
int multibody_com_batch_f32(const Multibody *mb, const float *q, float *com, int64_t batch, int64_t ld, void *stream) {
    return com_batch<float>(mb, false, q, com, batch, ld, stream);
}
int multibody_com_batch_f64(const Multibody *mb, const double *q, double *com, int64_t batch, int64_t ld,
                            void *stream) {
    return com_batch<double>(mb, false, q, com, batch, ld, stream);
}
int multibody_centroidal_batch_f32(const Multibody *mb, const float *q, const float *qd, float *com, float *hg,
                                   float *energy, int64_t batch, int64_t ld, void *stream) {
    return centroidal_batch<float>(mb, q, qd, com, hg, energy, batch, ld, stream);
}
int multibody_centroidal_batch_f64(const Multibody *mb, const double *q, const double *qd, double *com, double *hg,
                                   double *energy, int64_t batch, int64_t ld, void *stream) {
    return centroidal_batch<double>(mb, q, qd, com, hg, energy, batch, ld, stream);
}
int multibody_cmm_batch_f32(const Multibody *mb, const float *q, float *ag, int64_t batch, int64_t ld, void *stream) {
    return com_batch<float>(mb, true, q, ag, batch, ld, stream);
}
int multibody_cmm_batch_f64(const Multibody *mb, const double *q, double *ag, int64_t batch, int64_t ld,
                            void *stream) {
    return com_batch<double>(mb, true, q, ag, batch, ld, stream);
}
int multibody_com_batch_host_f32(const Multibody *mb, const float *q, float *com, int64_t batch) {
    return com_host<float>(mb, false, q, com, batch);
}
int multibody_com_batch_host_f64(const Multibody *mb, const double *q, double *com, int64_t batch) {
    return com_host<double>(mb, false, q, com, batch);
}
int multibody_centroidal_batch_host_f32(const Multibody *mb, const float *q, const float *qd, float *com, float *hg,
                                        float *energy, int64_t batch) {
    return centroidal_host<float>(mb, q, qd, com, hg, energy, batch);
}
int multibody_centroidal_batch_host_f64(const Multibody *mb, const double *q, const double *qd, double *com,
                                        double *hg, double *energy, int64_t batch) {
    return centroidal_host<double>(mb, q, qd, com, hg, energy, batch);
}
int multibody_cmm_batch_host_f32(const Multibody *mb, const float *q, float *ag, int64_t batch) {
    return com_host<float>(mb, true, q, ag, batch);
}
int multibody_cmm_batch_host_f64(const Multibody *mb, const double *q, double *ag, int64_t batch) {
    return com_host<double>(mb, true, q, ag, batch);
}

// Single configuration, fp64, on the calling thread (host_eval.cpp): multibody_link_pose's scope.
// which: 0 com (out0), 1 centroidal (out0 com, out1 hg, out2 energy), 2 cmm (out0).
static int centroidal_single(const Multibody *mb, int which, const double *q, const double *qd, double *out0,
                             double *out1, double *out2) {
    const std::string op = centroidal_name(which);
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (int rc = which == 1 ? centroidal_args_ok<double>(mb, 1, {q, qd}, {out0, out1, out2})
                            : centroidal_args_ok<double>(mb, which, {q}, {out0}))
        return rc;
    if (!mb->model.serial_revolute())
        return set_err(RB_ERR_UNSUPPORTED, op + ": the single-configuration form evaluates serial revolute chains only "
                                           "(kinematic trees, prismatic joints and a floating base take the batched "
                                           "entry points)");
    const double *pk = mb->pk64.data();
    const bool ok = which == 0   ? rbamd::host_com(mb->model, pk, q, out0)
                    : which == 1 ? rbamd::host_centroidal(mb->model, pk, q, qd, out0, out1, out2)
                                 : rbamd::host_cmm(mb->model, pk, q, out0);
    if (!ok)
        return set_err(RB_ERR_UNSUPPORTED, op + ": the single-configuration form runs on the host and needs an FMA3 / "
                                           "AVX2 CPU");
    return RB_OK;
}
int multibody_com(const Multibody *mb, const double *q, double *com) {
    return centroidal_single(mb, 0, q, nullptr, com, nullptr, nullptr);
}
int multibody_centroidal(const Multibody *mb, const double *q, const double *qd, double *com, double *hg,
                         double *energy) {
    return centroidal_single(mb, 1, q, qd, com, hg, energy);
}
int multibody_cmm(const Multibody *mb, const double *q, double *ag) {
    return centroidal_single(mb, 2, q, nullptr, ag, nullptr, nullptr);
}

// ------------------------------------------------------------- compliant ground contact
int multibody_contact_wrench_batch_f32(const Multibody *mb, const float *q, const float *qd, float *fext,
                                       float *cforce, int64_t batch, int64_t ld, void *stream) {
    return contact_wrench_batch<float>(mb, q, qd, fext, cforce, batch, ld, stream);
}
int multibody_contact_wrench_batch_f64(const Multibody *mb, const double *q, const double *qd, double *fext,
                                       double *cforce, int64_t batch, int64_t ld, void *stream) {
    return contact_wrench_batch<double>(mb, q, qd, fext, cforce, batch, ld, stream);
}
int multibody_contact_wrench_batch_host_f32(const Multibody *mb, const float *q, const float *qd, float *fext,
                                            float *cforce, int64_t batch) {
    return contact_wrench_host<float>(mb, q, qd, fext, cforce, batch);
}
int multibody_contact_wrench_batch_host_f64(const Multibody *mb, const double *q, const double *qd, double *fext,
                                            double *cforce, int64_t batch) {
    return contact_wrench_host<double>(mb, q, qd, fext, cforce, batch);
}
int multibody_rollout_contact_batch_f32(const Multibody *mb, float *q, float *qd, const float *tau_seq, double dt,
                                        int K, float *traj, int64_t batch, int64_t ld, void *stream) {
    return rollout_contact_batch<float>(mb, q, qd, tau_seq, dt, K, traj, batch, ld, stream);
}
int multibody_rollout_contact_batch_f64(const Multibody *mb, double *q, double *qd, const double *tau_seq, double dt,
                                        int K, double *traj, int64_t batch, int64_t ld, void *stream) {
    return rollout_contact_batch<double>(mb, q, qd, tau_seq, dt, K, traj, batch, ld, stream);
}
int multibody_rollout_contact_batch_host_f32(const Multibody *mb, float *q, float *qd, const float *tau_seq, double dt,
                                             int K, float *traj, int64_t batch) {
    return rollout_contact_host<float>(mb, q, qd, tau_seq, dt, K, traj, batch);
}
int multibody_rollout_contact_batch_host_f64(const Multibody *mb, double *q, double *qd, const double *tau_seq,
                                             double dt, int K, double *traj, int64_t batch) {
    return rollout_contact_host<double>(mb, q, qd, tau_seq, dt, K, traj, batch);
}

// Single configuration, fp64, on the calling thread (host_eval.cpp): multibody_rnea_ext's scope.
static int contact_single_scope(const Multibody *mb, const char *op) {
    if (!mb->model.serial_revolute())
        return set_err(RB_ERR_UNSUPPORTED, std::string(op) + ": the single-configuration form evaluates serial revolute "
                                           "chains only (kinematic trees, prismatic joints and a floating base take "
                                           "the batched entry points)");
    return RB_OK;
}
static int contact_single_no_fma(const char *op) {
    return set_err(RB_ERR_UNSUPPORTED, std::string(op) + ": the single-configuration form runs on the host and needs "
                                       "an FMA3 / AVX2 CPU");
}
int multibody_contact_wrench(const Multibody *mb, const double *q, const double *qd, double *fext, double *cforce) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (int rc = contact_args_ok<double>(mb, false, {q, qd}, {fext, cforce})) return rc;
    if (int rc = contact_single_scope(mb, "contact_wrench")) return rc;
    if (!rbamd::host_contact_wrench(mb->model, mb->pk64.data(), mb->ra64.data(), q, qd, fext, cforce))
        return contact_single_no_fma("contact_wrench");
    return RB_OK;
}
int multibody_rollout_contact(const Multibody *mb, double *q, double *qd, const double *tau_seq, double dt, int K,
                              double *traj) {
    if (!mb) return set_err(RB_ERR_NULL, "NULL Multibody handle");
    if (K < 0) return set_err(RB_ERR_ARG, "negative step count");
    if (K == 0) return RB_OK;
    if (int rc = contact_args_ok<double>(mb, true, {tau_seq}, {q, qd, traj})) return rc;
    if (int rc = contact_single_scope(mb, "rollout_contact")) return rc;
    if (!rbamd::host_rollout_contact(mb->model, mb->pk64.data(), mb->ra64.data(), q, qd, tau_seq, dt, K, traj))
        return contact_single_no_fma("rollout_contact");
    return RB_OK;
}

// ------------------------------------------------------------- batched (host)

int multibody_rnea_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                  double *tau, int64_t batch) {
    return rnea_host<double>(mb, q, qd, qdd, tau, batch);
}
int multibody_fd_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *tau,
                                double *qdd, int64_t batch) {
    return fd_host<double>(mb, q, qd, tau, qdd, batch);
}
int multibody_rnea_fd_batch_host_f64(const Multibody *mb, const double *q, const double *qd, const double *qdd,
                                     const double *tau_in, double *tau, double *qdd_out, int64_t batch) {
    return idfd_host<double>(mb, q, qd, qdd, tau_in, tau, qdd_out, batch);
}
int multibody_rnea_fd_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                     const float *tau_in, float *tau, float *qdd_out, int64_t batch) {
    return idfd_host<float>(mb, q, qd, qdd, tau_in, tau, qdd_out, batch);
}
int multibody_rnea_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *qdd,
                                  float *tau, int64_t batch) {
    return rnea_host<float>(mb, q, qd, qdd, tau, batch);
}
int multibody_fd_batch_host_f32(const Multibody *mb, const float *q, const float *qd, const float *tau,
                                float *qdd, int64_t batch) {
    return fd_host<float>(mb, q, qd, tau, qdd, batch);
}

// ------------------------------------------------------------- synthetic inputs

int rb_fill_uniform_f32(float *x, int n_rows, int64_t batch, int64_t ld, const double *lo, const double *hi,
                        uint64_t seed, void *stream) {
    return fill_uniform<float>(x, n_rows, batch, ld, lo, hi, seed, stream);
}
int rb_fill_uniform_f64(double *x, int n_rows, int64_t batch, int64_t ld, const double *lo, const double *hi,
                        uint64_t seed, void *stream) {
    return fill_uniform<double>(x, n_rows, batch, ld, lo, hi, seed, stream);
}

}  // extern "C"
