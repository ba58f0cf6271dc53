// jit.hpp -- model-specialised kernels compiled at model-load time with hipRTC.
//
// The precompiled kernels read the model's per-link constants from LDS, so every
// rotation entry and offset costs an FMA even when it is 0 or +-1.  URDF joint frames
// are usually signed axis permutations (rpy in multiples of pi/2) with sparse offsets;
// compiling the SAME device code (rnea_body.hip.hpp) against the model as a constexpr
// array lets the compiler fold those constants away (FR3 RNEA: ~1090 -> see DESIGN.md).
// Rotation/offset entries within 1e-14 of 0 or +-1 are snapped to exactly those values
// (the reference's own quaternion->matrix round trip leaves 1e-16 residues there), and
// the module is compiled with -ffinite-math-only -fno-signed-zeros so 0*x and 1*x fold.
//
// Any hipRTC failure leaves the precompiled generic kernel in charge (still on the GPU);
// RB_JIT=0 (or rb_set_tuning("jit", 0)) disables the path.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "model.hpp"

namespace rbamd {

// FwdKin / Jac: built only for models the precompiled kinematics kernels cannot express
// (kinematic trees, prismatic joints -- Model::serial_revolute() false).
// RneaFd: inverse + forward dynamics of the same (q, qd) in one launch (fdh_body.hip.hpp
// fdh_idfd_eval), for models on the mass-matrix forward dynamics (jit_fd_form 2).
// RneaDeriv / FdDeriv: analytical derivatives of the inverse / forward dynamics
// (rnea_deriv_body.hip.hpp), serial revolute chains only -- FdDeriv on the mass-matrix forward
// dynamics only (jit_kind_unsupported); they have no precompiled generic kernel.
// RolloutVjp: the reverse-mode gradient of the fused rollout (rollout_vjp_body.hip.hpp), FdDeriv's
// scope, hipRTC only.  Internal: the public kind numbers of the *_ex inspection queries end at 8
// (kJitPublicKinds); this kernel is inspected through multibody_rollout_vjp_jit_source / _compile.
// RneaExt / FdExt: inverse / forward dynamics under external link wrenches (ext_body.hip.hpp), every
// model, hipRTC only, one configuration per lane on SoA rows; FdExt takes the formulation
// jit_fd_form picks for Fd.  Internal too: multibody_ext_jit_source / _compile.
// LinkPose / LinkVel: pose / spatial velocity of every link in its URDF link frame
// (link_kin_body.hip.hpp), every model, hipRTC only, one configuration per lane on SoA rows.
// Internal too: multibody_link_kin_jit_source / _compile.
// ContactWrench / RolloutContact: the contact set's wrench, and the fused rollout under it
// (contact_body.hip.hpp), every model that carries a contact set (Model::contacts), hipRTC only, one
// configuration per lane on SoA rows; the set is compiled in and part of jit_key.  RolloutContact's
// forward dynamics follows jit_fd_form(m, JitKind::Rollout).  Internal too:
// multibody_contact_jit_source / _compile.
// RolloutContactVjp: the reverse-mode gradient of the contact rollout (contact_vjp_body.hip.hpp):
// RolloutVjp's scope on a model that carries a contact set, the set compiled in and part of jit_key.
// Internal too: multibody_contact_vjp_jit_source / _compile.
// Com / Centroidal / Cmm: centre of mass, centroidal momentum and energy, and the centroidal momentum
// matrix (centroidal_body.hip.hpp), every model with a positive total mass, hipRTC only, one
// configuration per lane on SoA rows.  Internal too: multibody_centroidal_jit_source / _compile.
// RneaVjp / RneaVjpExt: the reverse-mode gradient of the inverse dynamics without / with external link
// wrenches (rnea_vjp_body.hip.hpp), every model, hipRTC only, one configuration per lane on SoA rows.
// Internal too: multibody_rnea_vjp_jit_source / _compile.
// FdVjp / FdVjpExt: the reverse-mode gradient of the forward dynamics without / with external link
// wrenches (fd_vjp_body.hip.hpp), every model, hipRTC only, one configuration per lane on SoA rows; its
// forward stage takes the formulation jit_fd_form picks for Fd, as FdExt.  Internal too:
// multibody_fd_vjp_jit_source / _compile.
enum class JitKind : int {
    Rnea = 0, Fd = 1, Crba = 2, Rollout = 3, FwdKin = 4, Jac = 5, RneaFd = 6, RneaDeriv = 7, FdDeriv = 8,
    RolloutVjp = 9, RneaExt = 10, FdExt = 11, LinkPose = 12, LinkVel = 13, ContactWrench = 14, RolloutContact = 15,
    RolloutContactVjp = 16, Com = 17, Centroidal = 18, Cmm = 19, RneaVjp = 20, RneaVjpExt = 21,
    FdVjp = 22, FdVjpExt = 23
};
constexpr int kJitKinds = 24;
constexpr int kJitPublicKinds = 9;

// Why `kind` has no kernel for this model (empty: it has one).  Only the derivative kinds, the
// rollout's gradient, the contact kinds (a contact set) and the centroidal kinds (a positive total
// mass) are restricted here; jit_source returns an empty source for a model this refuses.
std::string jit_kind_unsupported(const Model &m, JitKind kind);

// One compiled kernel of a model: with the model and the tuning knobs (jit_key), everything its
// source and compile flags depend on.  jit_resolve is the only producer.
struct JitVariant {
    JitKind kind = JitKind::Rnea;
    bool f64 = false;
    bool fast = false;  // fp32 hardware sin / cos (v_sin_f32 / v_cos_f32); never set for fp64
    // the configurations-per-lane form the kernel really has: 1 one per lane, 2 paired fp32 lanes
    // (512 per block), 3 sequential pair, 4 / 5 the packed / one-per-lane wave split
    int pack = 1;
    int tail = 0;  // sequential-pair RNEA only: percent of the launch's tiles run one per lane (0 none)
    int nt = -1;   // the non-temporal load / store bits compiled in (RB_NT); -1 = the kind's tuning
};

struct JitKernel {
    hipModule_t module = nullptr;
    hipFunction_t function = nullptr;  // the lane kernel (any layout)
    JitVariant variant;                // what was built; jit_grid reads its pack and tail
    unsigned block = 256;              // threads per block
    std::string error;                 // non-empty when compilation failed
};

bool jit_enabled();

// The kernel variant a launch of B configurations of `kind` takes on this model (tiled: the
// [ceil(B/256)][n][256] layout): every batch-, layout- and model-dependent choice of lane form,
// tail, load / store policy and trig form is made here.  fast_trig: the process's fp32 trig
// flag (RB_FAST_TRIG).
JitVariant jit_resolve(const Model &m, JitKind kind, bool f64, uint32_t B, bool tiled, bool fast_trig);

// Cache key of a variant's kernel: the variant and every tuning value that changes the source
// or the compile flags (tuning.hpp).
std::string jit_key(const Model &m, const JitVariant &v);

// Generated HIP source for one specialised kernel (exposed for tests / inspection).
// waves: amdgpu_waves_per_eu target of the kernel; -1 = the policy (the jit_waves tuning and the
// per-form rules in jit_source).  jit_compile may rebuild with a 2-wave target (occupancy cliff,
// below).
std::string jit_source(const Model &m, const JitVariant &v, int waves);

// Blocks of a launch of B configurations on `jk` (the grid its source was written for).
unsigned jit_grid(const JitKernel &jk, uint32_t B);

// Unified VGPR count (arch VGPRs + AGPRs) of a code object's kernel, from its AMDGPU metadata;
// -1 if not found.
int code_vgprs(const std::vector<char> &code);

// Forward-dynamics algorithm for this model (tuning fd_form): 2 = mass-matrix method
// (fdh_body.hip.hpp), 1 = Articulated-Body Algorithm (aba_body.hip.hpp).
int jit_fd_form(const Model &m, JitKind kind = JitKind::Fd);

// hipRTC compilation only (no device needed): fills `code` with the code object.  Occupancy
// cliff: a kernel built without an occupancy target that lands just past 256 registers (one
// wave per SIMD, <= 16 over) is rebuilt with a 2-wave target -- a few spilled values cost less
// than half the SIMD's waves (the 9-joint tree's fp64 RNEA: 258 registers; 65.0 vs 92.9 us at
// 2^20 with 12 B of scratch; 234 registers at the first build once the kernel arguments are
// preloaded, tuning.hpp kernarg_preload).
// final_src (optional): the source of the code object returned -- the occupancy-cliff rebuild's
// when that rule applied (multibody_jit_source_ex reports this one).
bool jit_compile(const Model &m, const JitVariant &v, const std::string &arch, std::vector<char> *code,
                 std::string *error, std::string *final_src = nullptr);

// Compiles and loads the kernel on the current device.  Never throws.
JitKernel jit_build(const Model &m, const JitVariant &v);

}  // namespace rbamd
