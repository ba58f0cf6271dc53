// jit.cpp -- see jit.hpp.
#include "jit.hpp"

#include <hip/hiprtc.h>

#include <algorithm>
#include <string_view>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <vector>

#include "jit_sources.inc"  // kJitHeaderNames / kJitHeaderSources (tools/embed_sources.py)
#include "layout.hpp"
#include "tuning.hpp"

namespace rbamd {

bool jit_enabled() { return tuning().jit != 0; }

namespace {

double snap(double x) {
    if (std::fabs(x) < 1e-14) return 0.0;
    if (std::fabs(x - 1.0) < 1e-14) return 1.0;
    if (std::fabs(x + 1.0) < 1e-14) return -1.0;
    return x;
}

std::string literal(double x, bool f64) {
    char buf[64];
    if (x == 0.0) return f64 ? "0.0" : "0.0f";
    if (f64)
        std::snprintf(buf, sizeof buf, "%.17g", x);
    else
        std::snprintf(buf, sizeof buf, "%.9gf", (double)(float)x);
    std::string s(buf);
    // make sure an integral value still reads as a floating literal
    if (s.find_first_of(".eEn") == std::string::npos) s.insert(f64 ? s.size() : s.size() - 1, ".0");
    return s;
}

// ---- policy: which kernel variant a launch takes (jit_resolve) and what each variant's source
// and compile flags are made of.  Every tuning knob read here is part of jit_key.

int jit_nt(JitKind kind) {
    // (the external-wrench kinds follow their plain neighbours: every row is touched once)
    if (kind == JitKind::Rnea || kind == JitKind::RneaExt || kind == JitKind::RneaVjp || kind == JitKind::RneaVjpExt)
        return tuning().rnea_nt < 0 ? 3 : (tuning().rnea_nt & 3);
    if (kind == JitKind::Fd || kind == JitKind::Rollout || kind == JitKind::RneaFd || kind == JitKind::FdExt ||
        kind == JitKind::RolloutContact || kind == JitKind::FdVjp || kind == JitKind::FdVjpExt)
        return tuning().fd_nt & 3;
    // CRBA, fwd_kin, jac, link_pose / link_vel, contact_wrench and cmm (output-bound, as jac)
    if (kind == JitKind::Com || kind == JitKind::Centroidal) return tuning().kin_nt >= 0 ? tuning().kin_nt & 3 : 3;  // as fwd_kin
    const int v = tuning().kin_nt;
    if (v >= 0) return v & 3;
    return kind == JitKind::FwdKin ? 3 : 2;  // 7 rows in / 3 out: non-temporal loads pay too
}

// Rollouts whose K loop must not hoist anything (machine LICM off, the row stride re-derived
// per step): the paired fp32 form, and fp64 chains up to 8 links -- 212 instead of 264 VGPRs,
// 2 waves/SIMD instead of 1: FR3 2^20 x 16 steps 641 vs 1027 us (12 links: no change; 30
// links, state in registers: 6.09 vs 5.81 ms, so not there).
bool jit_rollout_no_hoist(bool f64, int n, int pack) { return pack == 2 || pack == 4 || (f64 && n <= 8); }

bool jit_opaque(JitKind kind, bool f64, int n) {
    const int v = tuning().opaque_consts;
    if (v >= 0) return v != 0;
    // fp64 short-chain rollouts: with hoisting off, SGPR-pinned fp64 constants only spill
    return n <= 16 && kind == JitKind::Rollout && !(f64 && n <= 8);
}

// Configurations per lane of `kind`'s lane kernel under the tuning `pack` alone (jit_resolve
// adds the batch rules, jit_model_pack what the model allows).
int jit_pack(JitKind kind, bool f64, int n) {
    // 2 = two configurations per lane on packed fp32 (fp32 forward dynamics of chains up to 8
    // links: FR3 2^20 tiled 28.7 vs 30.7 us; 200+ VGPRs for the pair, 2 waves/SIMD; the
    // 30-link chain needs ~240 VGPRs for one configuration).  The RNEA pair (128 VGPRs, 4
    // waves/SIMD instead of 8) measured slower, 22.6 vs 21.0 us, and was removed.  The fp32
    // rollout of chains up to 8 links is paired too (rollout_lane2: 251 VGPRs, 2 waves/SIMD,
    // constants pinned in SGPRs and machine LICM off so the K loop hoists nothing; FR3 2^20
    // x 16 steps 317-323 vs 333-335 us one per lane at 4 waves/SIMD).
    // 3 = two configurations per lane evaluated one after the other from one load burst (the
    // fp64 RNEA of chains up to 8 links: 125 VGPRs, still 4 waves/SIMD; FR3 2^20 tiled
    // 42.0-42.8 us steady where the one-per-lane kernel alternates between ~40.7 and ~48.8 us
    // phases, mean 44.3-44.6).
    const int v = tuning().pack;
    if (kind == JitKind::Rollout) return ((v < 0 || v == 2 || v == 4) && !f64 && n <= 8) ? (v == 4 ? 4 : 2) : 1;
    // the fused inverse + forward dynamics: one per lane, or its wave split (idfd_split_block1)
    if (kind == JitKind::RneaFd) return v == 5 ? 5 : 1;
    if (kind != JitKind::Fd && kind != JitKind::Rnea) return 1;
    if (v == 3) return 3;
    if (v == 4) return (kind == JitKind::Fd && !f64) ? 4 : 1;  // split packed waves (fdh_split_block2)
    if (v == 5) return kind == JitKind::Fd ? 5 : 1;             // split waves, one per lane (fdh_split_block1)
    if (v >= 0) return (v >= 2 && !f64 && kind == JitKind::Fd) ? 2 : 1;
    if (kind == JitKind::Rnea) return (f64 && n <= 8) ? 3 : 1;
    return (!f64 && n <= 8) ? 2 : 1;
}

int jit_waves(JitKind kind, bool f64, int n) {
    const int v = tuning().jit_waves;
    if (v >= 0) return v;
    if (kind == JitKind::Rollout && !f64 && n <= 8) return jit_pack(kind, f64, n) != 1 ? 2 : 4;
    // (the fp64 rollout of the mass-matrix form takes a 4-wave target in jit_source; the ABA
    // form -- the rollout of trees, or fd_form 1 -- none: 436 B of scratch per lane under it)
    return 0;
}

bool jit_f64_tab(bool f64) { return f64 && tuning().f64_tab != 0; }

// Percent of a sequential-pair RNEA launch's tiles run one per lane for this layout (tuning
// seq_tail; auto: 75 for the tiled layout, 0 for SoA).
int jit_seq_tail(bool tiled) {
    const int v = tuning().seq_tail;
    if (v < 0) return tiled ? 75 : 0;
    return v < 100 ? v : 100;
}

// What the model-dependent rules below read of the model.  jit_resolve runs on every launch and
// serial_revolute() walks the links, so it is read once per resolve.
struct ModelShape {
    int n;
    bool serial;
};

int fd_form(const ModelShape &m, JitKind kind) {
    // 2 = mass-matrix forward dynamics (fdh_body.hip.hpp: RNEA bias + CRBA + L D L^T), 1 = the
    // Articulated-Body Algorithm (aba_body.hip.hpp).  The mass-matrix form holds ~n^2/2 values
    // per lane where the ABA holds ~12 per link across its sweeps, so it runs at 2-3x the
    // ABA's waves per SIMD on short chains; its O(n^2) work loses on long ones.  Trees keep
    // the ABA (tree_body.hip.hpp).  Forward dynamics: the mass-matrix form up to 12 links (12
    // links 2^20 tiled: fp64 119.0 vs 159.5 us on the ABA -- 242 registers, 2 waves/SIMD, against
    // the ABA's 398, 1 wave -- fp32 64.6 vs 75.6; 16 links: the ABA, 224 vs 229 / 101 vs 113;
    // profiles/r05/ab/fd_form/).  Rollouts: up to 8 links (12 links x 16 steps: the ABA 2205 vs
    // 3141 us fp64, 920 vs 959 fp32).
    const int v = tuning().fd_form;
    // trees: the mass-matrix form only for forward dynamics and only on request (fdh_eval_tree;
    // A/B), rollouts and the wave splits / pairs are serial-chain forms
    if (!m.serial) return (kind == JitKind::Fd && v == 2) ? 2 : 1;
    if (v == 1 || v == 2) return v;
    return m.n <= (kind == JitKind::Rollout ? 8 : 12) ? 2 : 1;
}

}  // namespace

int jit_fd_form(const Model &m, JitKind kind) { return fd_form({m.n, m.serial_revolute()}, kind); }

std::string jit_kind_unsupported(const Model &m, JitKind kind) {
    if (kind == JitKind::ContactWrench || kind == JitKind::RolloutContact)
        return m.contacts.n_points > 0 ? "" : std::string(kind == JitKind::ContactWrench ? "contact_wrench" : "rollout_contact") +
               ": the model carries no contact set (multibody_with_contacts makes a handle that does)";
    if (kind == JitKind::Com || kind == JitKind::Centroidal || kind == JitKind::Cmm)
        return m.total_mass() > 0 ? "" : std::string(kind == JitKind::Com ? "com" : kind == JitKind::Cmm ? "cmm" : "centroidal") +
               ": the model has no mass (the centre of mass is undefined)";
    if (kind == JitKind::RolloutContactVjp && m.contacts.n_points < 1)
        return "rollout_contact_vjp: the model carries no contact set (multibody_with_contacts makes a handle that does)";
    if (kind != JitKind::RneaDeriv && kind != JitKind::FdDeriv && kind != JitKind::RolloutVjp &&
        kind != JitKind::RolloutContactVjp)
        return "";
    const char *name = kind == JitKind::RneaDeriv ? "rnea_deriv" : kind == JitKind::FdDeriv ? "fd_deriv"
                       : kind == JitKind::RolloutVjp ? "rollout_vjp" : "rollout_contact_vjp";
    if (!m.serial_revolute())
        return std::string(name) + ": no such kernel for this model: serial revolute chains only (kinematic trees, "
               "prismatic joints and a floating base are not supported)";
    if (kind != JitKind::RneaDeriv && jit_fd_form(m, JitKind::Fd) != 2)
        return std::string(name) + ": no such kernel for this model: it needs the mass-matrix forward dynamics "
               "(serial chains up to 12 links, fd_form 2); this model has " + std::to_string(m.n) +
               " links on the articulated-body form";
    return "";
}

namespace {

// The lane form a kernel of this model really takes for the requested pack (0 = the jit_pack policy).
int jit_model_pack(const ModelShape &m, JitKind kind, bool f64, int pack_req) {
    const int pack = pack_req > 0 ? pack_req : jit_pack(kind, f64, m.n);
    if (kind == JitKind::Fd) {
        const bool fdh = fd_form(m, kind) == 2;
        // the tree form of the mass-matrix forward dynamics is one configuration per lane
        if (!m.serial && fdh) return 1;
        // the mass-matrix forward dynamics has one- and two-per-lane forms only
        if (pack == 3 && fdh) return 1;
    }
    // 4 / 5 = the bias / mass-matrix wave split, packed / one per lane: fp32 mass-matrix FD only
    if (pack == 4 && kind == JitKind::Rollout && !(!f64 && fd_form(m, kind) == 2 && !(tuning().jit_variant & 256)))
        return (!f64 && m.n <= 8) ? 2 : 1;  // the split needs the mass-matrix form: the pair instead
    if (pack == 4 && kind != JitKind::Rollout && !(kind == JitKind::Fd && !f64 && fd_form(m, JitKind::Fd) == 2)) return 1;
    if (pack == 5 && !((kind == JitKind::Fd || kind == JitKind::RneaFd) && fd_form(m, JitKind::Fd) == 2 && m.serial))
        return 1;
    return pack;
}

// ---- the lane form a launch of B configurations asks for while the tuning `pack` is unset
// (the auto policy); 0 = the jit_pack policy.  jit_model_pack then clamps it to the model.

// Smallest batch for which the auto policy takes the sequential-pair fp64 RNEA (jit_pack 3):
// it halves the waves, so below two resident rounds of the one-per-lane kernel (4 waves/SIMD x
// 1024 SIMDs x 64 lanes x 2) the one-per-lane kernel keeps more of the chip busy.
constexpr uint32_t kSeqMinBatch = 1u << 19;

// fp32 chains up to 8 links on the tiled layout at large batches: the sequential pair too
// (FR3 2^20 22.0-22.1 vs 22.3-24.0 us on two boxes, profiles/r04/ab/ab_r32_seq*.log), with
// ordinary (temporal) loads and stores (tuning.hpp rnea_nt; the 30-link chain and the 14-DOF
// tree keep nt = 3)
bool rnea_big32(const ModelShape &m, bool f64, uint32_t B, bool tiled) {
    return !f64 && tiled && B >= kSeqMinBatch && m.n <= 8;
}

int rnea_pack(const ModelShape &m, bool f64, uint32_t B, bool tiled) {
    return tuning().pack >= 0 ? 0 : rnea_big32(m, f64, B, tiled) ? 3 : B < kSeqMinBatch ? 1 : 0;
}

// Smallest batch for which the auto policy takes the paired-lane kernel: one resident round
// of it (2 blocks of 512 configurations per CU x 256 CUs) -- 2^18.
constexpr uint32_t kPackMinBatch = 1u << 18;
// fp32 mass-matrix forward dynamics at small batches: one wave per SIMD at most, so the launch
// time follows each wave's instruction stream; the wave splits (fdh_body.hip.hpp) halve it.
// Up to 2^17 configurations the one-per-lane split (pack 5: B/32 waves, its roles alternating
// over the SIMDs), above it the packed pair; the packed split (pack 4: B/64 waves) is the
// rollout's, with the same bound.  FR3, HIP graph (profiles/r06/mix/): 32768 3.53 us (pack 5)
// / 3.99 (4); 65536 4.15 (5) / 4.24 (4); 131072 5.45 (5) / 5.50 (4).
constexpr uint32_t kSplitMaxBatch = 1u << 17;

// The forward-dynamics kernel a launch of B configurations takes (auto policy when the
// tuning `pack` is unset).
int fd_pack(const ModelShape &m, bool f64, uint32_t B) {
    int pack = 0;
    if (tuning().pack < 0) {
        if (!f64 && fd_form(m, JitKind::Fd) == 2 && m.n <= 8 && m.serial)  // splits: serial chains, measured on FR3
            pack = B <= kSplitMaxBatch ? 5 : 0;
        else  // paired lanes halve the grid: below kPackMinBatch one per lane fills more CUs
            pack = B < kPackMinBatch ? 1 : 0;
    }
    return pack;
}

// The rollout kernel a launch of B configurations takes: fp32 mass-matrix rollouts up to 2^17
// configurations split every step over a pair of packed waves (aba_body.hip.hpp
// rollout_split_block2), as fd_pack's small-batch forward dynamics.  FR3, K = 16, HIP graph:
// 16384 43.3 vs 62.7 us (pair), 65536 43.6 vs 63.5, 131072 58.9 vs 63.7; 262144 101.5 vs 93.2
// (profiles/r03/rollout_split/).
int rollout_pack(const ModelShape &m, bool f64, uint32_t B) {
    return (tuning().pack < 0 && !f64 && B <= kSplitMaxBatch && fd_form(m, JitKind::Rollout) == 2 &&
            !(tuning().jit_variant & 256)) ? 4 : 0;
}

// The fused pair's kernel form for B configurations (auto policy when the tuning `pack` is
// unset): the wave split (pack 5, idfd_split_block1) for fp32 up to 2^16 configurations, one
// per lane otherwise.  FR3, HIP graph, tiled (profiles/r06/split/): fp32 65536 4.82 vs 5.24 us,
// 131072 6.79 vs 6.49; fp64 65536 6.64 vs 6.70, 131072 11.55 vs 10.67, 262144 22.06 vs 20.59 --
// as for the forward dynamics alone (fp64 FD split 10.16 vs 8.62 us at 2^17): the SIMDs already
// hold 2 waves of the one-per-lane kernel there, and the split repeats the loads and sincos.
// With the split's roles alternating over the SIMDs (round 6, profiles/r06/mix/): fp32 65536
// 4.75 us, 131072 6.53 vs 6.46 one per lane -- the bound stays.
constexpr uint32_t kIdfdSplitMaxBatch32 = 1u << 16;
int idfd_pack(bool f64, uint32_t B) {
    if (tuning().pack >= 0) return 0;
    return (!f64 && B <= kIdfdSplitMaxBatch32) ? 5 : 1;
}

}  // namespace

JitVariant jit_resolve(const Model &model, JitKind kind, bool f64, uint32_t B, bool tiled, bool fast_trig) {
    // only the forward-dynamics kinds' rules read `serial`: the others do not pay for the walk
    const bool fd_kind = kind == JitKind::Fd || kind == JitKind::Rollout || kind == JitKind::RneaFd;  // (the
    // derivative kinds are one configuration per lane whatever the model: jit_pack, jit_model_pack)
    const ModelShape m{model.n, fd_kind && model.serial_revolute()};
    JitVariant v;
    v.kind = kind;
    v.f64 = f64;
    // CRBA evaluates its angles with the precise fp32 sincos; every other kind with the fast one
    // unless RB_FAST_TRIG=0 (fp64 always its own)
    v.fast = kind != JitKind::Crba && fast_trig && !f64;
    int pack_req = 0;
    switch (kind) {
        case JitKind::Rnea:
            pack_req = rnea_pack(m, f64, B, tiled);
            v.nt = (rnea_big32(m, f64, B, tiled) && tuning().rnea_nt < 0) ? 0 : -1;
            break;
        case JitKind::Fd: pack_req = fd_pack(m, f64, B); break;
        case JitKind::Rollout: pack_req = rollout_pack(m, f64, B); break;
        case JitKind::RneaFd: pack_req = idfd_pack(f64, B); break;
        default: break;
    }
    v.pack = jit_model_pack(m, kind, f64, pack_req);
    if (kind == JitKind::Rnea && v.pack == 3) v.tail = jit_seq_tail(tiled);
    return v;
}

// The contact set as key text: a different set is a different kernel (exact values, hex floats).
static std::string contact_key(const ContactSet &c) {
    char buf[32];
    std::string s = ":c" + std::to_string(c.n_points);
    auto add = [&](double x) {
        std::snprintf(buf, sizeof buf, ",%a", x);
        s += buf;
    };
    for (int p = 0; p < c.n_points; ++p) {
        s += "," + std::to_string(c.link[p]);
        for (int k = 0; k < 3; ++k) add(c.point[p][k]);
    }
    for (int k = 0; k < 3; ++k) add(c.normal[k]);
    for (double x : {c.offset, c.stiffness, c.damping, c.friction, c.slip_velocity}) add(x);
    return s;
}

std::string jit_key(const Model &m, const JitVariant &v) {
    const JitKind kind = v.kind;
    const bool f64 = v.f64;
    const bool contact = kind == JitKind::ContactWrench || kind == JitKind::RolloutContact ||
                         kind == JitKind::RolloutContactVjp;
    // ":w" the policy's target, ":W" the raw knob (-1 lets jit_compile rebuild at the occupancy cliff)
    return ":k" + std::to_string((int)kind) + (f64 ? ":f64" : ":f32") + (v.fast ? ":fast" : ":precise") + ":nt" +
           std::to_string(jit_nt(kind)) + ":w" + std::to_string(jit_waves(kind, f64, m.n)) + ":W" +
           std::to_string(tuning().jit_waves.load()) + ":o" +
           std::to_string(jit_opaque(kind, f64, m.n) ? 1 : 0) + ":p" + std::to_string(jit_pack(kind, f64, m.n)) +
           ":t" + std::to_string(jit_f64_tab(f64) ? 1 : 0) + ":r" + std::to_string(tuning().split_rot) + ":v" +
           std::to_string(tuning().jit_variant) + ":f" + std::to_string(tuning().fd_form) + ":k" +
           std::to_string(kind == JitKind::Rnea ? tuning().rnea_park.load() : 0) + ":e" +
           std::to_string(kind == JitKind::Rnea ? tuning().rnea_rev.load() : 0) + ":a" +
           std::to_string(tuning().kernarg_preload.load()) + ":q" + std::to_string(v.pack) + ":st" +
           std::to_string(v.tail) + ":n" + std::to_string(v.nt) + (contact ? contact_key(m.contacts) : std::string());
}

int code_vgprs(const std::vector<char> &code) {
    // msgpack map entry ".vgpr_count" (fixstr 0xab) -> positive fixint / uint8 (0xcc) / uint16 (0xcd)
    static const char key[] = "\xab.vgpr_count";
    const std::string_view buf(code.data(), code.size());
    const size_t at = buf.find(std::string_view(key, sizeof(key) - 1));
    if (at == std::string_view::npos) return -1;
    size_t i = at + sizeof(key) - 1;
    if (i >= buf.size()) return -1;
    const unsigned char t = (unsigned char)buf[i];
    if (t < 0x80) return t;
    if (t == 0xcc && i + 1 < buf.size()) return (unsigned char)buf[i + 1];
    if (t == 0xcd && i + 2 < buf.size()) return ((unsigned char)buf[i + 1] << 8) | (unsigned char)buf[i + 2];
    return -1;
}

// The paired fp32 rollout and the fp64 rollout of short chains keep 2 waves/SIMD only
// without machine LICM: hoisting per-step address arithmetic and constants out of the K
// loop costs the VGPRs below 256 (fp64 FR3: 212 instead of 264).
static bool jit_no_licm(const Model &m, const JitVariant &v) {
    return v.kind == JitKind::Rollout && jit_rollout_no_hoist(v.f64, m.n, v.pack);
}

// The rollout's gradient is built without the SLP vectorizer: it pairs the fp32 column sweeps'
// independent FMAs into 2-wide operations whose register pairs cost more than the packed
// arithmetic saves (FR3 fp32: 512 registers and 840 B of scratch per lane with it, 194 and none
// without; fp64 380 / 386, no scratch either way).
static bool jit_no_slp(const JitVariant &v) {
    return v.kind == JitKind::RolloutVjp || v.kind == JitKind::RolloutContactVjp;
}

std::string jit_source(const Model &m, const JitVariant &v, int waves_req) {
    const JitKind kind = v.kind;
    const bool f64 = v.f64;
    const int pack = v.pack;
    const bool deriv = kind == JitKind::RneaDeriv || kind == JitKind::FdDeriv;
    const bool cvjp = kind == JitKind::RolloutContactVjp;  // the contact rollout's adjoint (contact_vjp_body.hip.hpp)
    const bool vjp = kind == JitKind::RolloutVjp || cvjp;  // the rollouts' adjoints: fd_deriv's scope and link forces
    const bool ext = kind == JitKind::RneaExt || kind == JitKind::FdExt;  // external link wrenches (ext_body.hip.hpp)
    const bool lk = kind == JitKind::LinkPose || kind == JitKind::LinkVel;  // every link's kinematics (link_kin_body.hip.hpp)
    // the contact set's wrench / the fused rollout under it (contact_body.hip.hpp).  RolloutContact
    // deliberately takes none of Rollout's tuned build rules below (no-hoist / machine LICM off, the
    // guard anchor below nine links, opaque constants, the fp64 4-wave target): each was adopted on an
    // A/B measurement of that kernel, none has been measured for this one.
    const bool contact = kind == JitKind::ContactWrench || kind == JitKind::RolloutContact || cvjp;
    // centre of mass, centroidal momentum / energy, momentum matrix (centroidal_body.hip.hpp)
    const bool cz = kind == JitKind::Com || kind == JitKind::Centroidal || kind == JitKind::Cmm;
    // the inverse dynamics' reverse-mode gradient (rnea_vjp_body.hip.hpp), without / with wrench rows
    const bool rvjp = kind == JitKind::RneaVjp || kind == JitKind::RneaVjpExt;
    // the forward dynamics' reverse-mode gradient (fd_vjp_body.hip.hpp), without / with wrench rows: built
    // as FdExt is (the same link-force form and forward-dynamics form), so its qdd is that kernel's
    const bool fvjp = kind == JitKind::FdVjp || kind == JitKind::FdVjpExt;
    if ((deriv || vjp || contact || cz) && !jit_kind_unsupported(m, kind).empty()) return "";
    std::vector<double> pk = m.pack_f64();
    for (int i = 0; i < m.n; ++i) {
        double *c = &pk[(size_t)i * kLinkStride];
        for (int k = 0; k < 9; ++k) c[kE0 + k] = snap(c[kE0 + k]);
        for (int k = 0; k < 3; ++k) c[kP + k] = snap(c[kP + k]);
    }
    const char *F = v.fast ? "true" : "false";

    // ---- what this variant's source is made of, decided before any text is written
    // (FdDeriv exists on the mass-matrix form only and must define what the Fd kernel defines:
    // its qdd is that kernel's, bit for bit)
    const bool fdh = (kind == JitKind::Fd || kind == JitKind::RneaFd || kind == JitKind::FdDeriv) && jit_fd_form(m) == 2;
    // the rollout's forward dynamics follows the fd_form policy (mass-matrix form for short
    // serial chains) unless RB_VARIANT bit 8 (A/B) keeps the ABA
    const bool rollout_fdh = kind == JitKind::Rollout && jit_fd_form(m, kind) == 2 && !(tuning().jit_variant & 256);
    const bool tab = jit_f64_tab(f64);
    // Split joint rotation (artinertia.hip.hpp to_parent_split): pays only when every R_p is a
    // signed permutation (its congruence then folds away); a dense constant R_p (general-axis
    // frames, trees) makes it costlier than the folded E S E^T.
    bool perm = true;
    for (int i = 0; i < m.n && perm; ++i)
        for (int r = 0; r < 3; ++r) {
            int ones = 0;
            for (int c = 0; c < 3; ++c) {
                const double e = pk[(size_t)i * kLinkStride + kE0 + 3 * r + c];
                if (e == 1.0 || e == -1.0) ++ones;
                else if (e != 0.0) perm = false;
            }
            if (ones != 1) perm = false;
        }
    const int sr = tuning().split_rot;
    const bool split_rot = sr > 0 || (sr < 0 && perm);
    // Newton-Euler link forces about the centre of mass (spatial.hip.hpp link_force) for the
    // RNEA sweeps of chains and trees (and so the mass-matrix FD's bias): c = h / m and
    // Ic = I_o - m (|c|^2 1 - c c^T) per link (massless virtual links: c = 0, Ic = I_o = 0), in
    // fp64 here.  jit_variant bit 9 (A/B) keeps the origin form.  Not for the fp64 RNEA of chains
    // up to 8 links (the reversed long-chain form below takes it): the
    // memory-bound headline kernel gains nothing from fewer VALU, its sequential pair would need
    // 131 instead of 125 VGPRs (3 waves/SIMD instead of 4), and all its grid forms (pairs,
    // single tail, one per lane below 2^19) must stay bit-identical to each other.
    const bool dyn = kind == JitKind::Rnea || kind == JitKind::Fd || kind == JitKind::Rollout || kind == JitKind::RneaFd ||
                     deriv || vjp || ext || fvjp || kind == JitKind::RolloutContact;
    // jit_variant bit 16384 (A/B): the centre-of-mass form for the fp64 RNEA too
    // rnea_lane_rev: the fp64 RNEA of serial chains longer than 8 links, whose per-link forces
    // hold one wave per SIMD (12 links 264 VGPRs, 30 links 496) and do not fit LDS either
    // (rnea_park's fp64 forces would take 60 KB per wave); centre-of-mass link forces, any joint
    // frames (general axes included)
    const bool rev = kind == JitKind::Rnea && f64 && m.n > 8 && m.serial_revolute() && tuning().rnea_rev != 0;
    const bool com = dyn && !(kind == JitKind::Rnea && f64 && !rev && !(tuning().jit_variant & 16384)) &&
                     !(tuning().jit_variant & 512);
    // rnea_lane_park: fp32 one-per-lane RNEA of long serial chains in the centre-of-mass g-form
    // (signed-permutation frames), when the tuning asks for it
    // the parked forces take NP x 6 KB of LDS per 4-wave block: at most kMaxPark links, so that 3
    // blocks still fit a CU's 160 KB (gfx950) -- a requested count past it is clamped, not handed to
    // hipRTC to fail on (which would leave the launch on the generic kernel)
    constexpr int kMaxPark = (160 * 1024 / 3) / (4 * 6 * 64 * 4);
    const int pk_req = std::min(kMaxPark, tuning().rnea_park < 0 ? (m.n >= 20 ? 8 : 0) : tuning().rnea_park.load());
    const int park = (kind == JitKind::Rnea && !f64 && pack == 1 && m.serial_revolute() && com && split_rot &&
                      pk_req > 0 && pk_req < m.n) ? pk_req : 0;
    // The occupancy target: a request, else the jit_waves policy, else (the knob unset) 4 for
    // three forms.  The paired mass-matrix FD fits 4 waves/SIMD at exactly 128 VGPRs with the
    // occupancy target (130 and 3 waves without): FR3 2^20 tiled 26.4 vs 27.0 us.
    int waves = waves_req >= 0 ? waves_req : jit_waves(kind, f64, m.n);
    const bool waves_auto = tuning().jit_waves < 0 && waves_req < 0;
    if (fdh && pack == 2 && waves_auto) waves = 4;
    // fp64 rollout of the mass-matrix form: 127 VGPRs, 4 waves/SIMD either way since the input
    // checks; the target keeps it there (FR3 2^20 x 16 steps, reset state: 690-708 vs 702-704 us,
    // noise-level).  Not for the ABA form: 256 VGPRs at 1 wave/SIMD runs 984 us, 2 / 3 / 4-wave
    // targets spill (1068 / 2756 / 4131 us; profiles/r05/ab/rollout_forms/).
    if (rollout_fdh && f64 && m.n <= 8 && waves_auto) waves = 4;
    if (kind == JitKind::Rnea && f64 && (tuning().jit_variant & 32768) && waves_auto) waves = 4;  // A/B
    // the parked kernel's own target, whatever was asked.  park > 0 means fp32 and pack 1, so
    // neither the reversed form (fp64) nor the sequential pair is emitted instead of it.
    if (park > 0) waves = 3;

    std::ostringstream o;
    o << "#define RB_NT " << (v.nt >= 0 ? v.nt : jit_nt(kind)) << "\n";
    o << "#define RB_VARIANT " << tuning().jit_variant << "\n";
    o << "#define RB_OPAQUE_CONSTS " << (jit_opaque(kind, f64, m.n) ? 1 : 0) << "\n";
    if (jit_no_licm(m, v)) o << "#define RB_ROLLOUT_NO_HOIST 1\n";
    // input checks pinned into the sweep's state (rnea_body.hip.hpp rnea_fwd)
    if (kind == JitKind::Rollout || m.n > 8) o << "#define RB_GUARD_ANCHOR 1\n";
    if (rollout_fdh) o << "#define RB_ROLLOUT_FDH 1\n";
    o << "#define RB_SINCOS_TAB " << (tab ? 1 : 0) << "\n";
    if (tab) {  // (cos, sin)(k pi/128), k < 256, for sincos_tab (spatial.hip.hpp): long double, quadrants exact
        const long double pi = 3.141592653589793238462643383279502884L;
        o << "static __device__ constexpr double rb_sctab_src[512] = {\n";
        for (int k = 0; k < 256; ++k) {
            double c = (double)std::cos((long double)k * pi / 128.0L), s = (double)std::sin((long double)k * pi / 128.0L);
            if (k % 64 == 0) {
                const int q = k / 64;
                c = q == 0 ? 1.0 : q == 2 ? -1.0 : 0.0;
                s = q == 1 ? 1.0 : q == 3 ? -1.0 : 0.0;
            }
            o << "  " << literal(c, true) << ", " << literal(s, true) << ",\n";
        }
        o << "};\n";
    }
    o << "#define RB_SPLIT_ROT " << (split_rot ? 1 : 0) << "\n";
    if (com) {
        o << "#define RB_COM_FORM 1\n";
        o << "static __device__ constexpr double rb_com[" << 9 * m.n << "] = {\n";
        for (int i = 0; i < m.n; ++i) {
            const double *L = &pk[(size_t)i * kLinkStride];
            const double mass = L[kM];
            double c[3] = {0, 0, 0};
            if (mass > 0)
                for (int k = 0; k < 3; ++k) c[k] = L[kH + k] / mass;
            const double cc = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
            const double Ic[6] = {L[kIo + 0] - mass * (cc - c[0] * c[0]), L[kIo + 1] + mass * c[0] * c[1],
                                  L[kIo + 2] + mass * c[0] * c[2],        L[kIo + 3] - mass * (cc - c[1] * c[1]),
                                  L[kIo + 4] + mass * c[1] * c[2],        L[kIo + 5] - mass * (cc - c[2] * c[2])};
            o << "  ";
            for (int k = 0; k < 3; ++k) o << literal(c[k], true) << ", ";
            for (int k = 0; k < 6; ++k) o << literal(Ic[k], true) << ", ";
            o << "\n";
        }
        o << "};\n";
    }
    o << (cvjp                                              ? "#include \"contact_vjp_body.hip.hpp\"\n"
          : contact                                         ? "#include \"contact_body.hip.hpp\"\n"
          : cz                                              ? "#include \"centroidal_body.hip.hpp\"\n"
          : rvjp                                            ? "#include \"rnea_vjp_body.hip.hpp\"\n"
          : fvjp                                            ? "#include \"fd_vjp_body.hip.hpp\"\n"
          : lk                                              ? "#include \"link_kin_body.hip.hpp\"\n"
          : ext                                             ? "#include \"ext_body.hip.hpp\"\n"
          : vjp                                            ? "#include \"rollout_vjp_body.hip.hpp\"\n"
          : deriv                                           ? "#include \"rnea_deriv_body.hip.hpp\"\n"
          : kind == JitKind::Rnea                             ? "#include \"rnea_body.hip.hpp\"\n"
          : fdh                                               ? "#include \"fdh_body.hip.hpp\"\n"
          : (kind == JitKind::Fd || kind == JitKind::Rollout) ? "#include \"aba_body.hip.hpp\"\n"
          : kind == JitKind::Crba                             ? "#include \"crba_body.hip.hpp\"\n"
                                                              : "#include \"tree_body.hip.hpp\"\n");
    o << "using T = " << (f64 ? "double" : "float") << ";\n";
    o << "constexpr int N = " << m.n << ";\n";
    // Topology policy (tree_body.hip.hpp): the tuned serial code for the reference's chain,
    // else the tree forms with every parent index / joint type a compile-time constant.
    if (m.serial_revolute()) {
        o << "using Topo = rbamd::dev::SerialTopo;\n";
    } else {
        o << "struct Topo {\n  static constexpr bool kSerial = false;\n  static constexpr int kPar[N] = {";
        for (int i = 0; i < m.n; ++i) o << (i ? ", " : "") << m.links[i].parent;
        o << "};\n  static constexpr int kPri[N] = {";
        for (int i = 0; i < m.n; ++i) o << (i ? ", " : "") << (m.links[i].type == kJointPrismatic ? 1 : 0);
        o << "};\n"
             "  static constexpr int parent(int j) { return kPar[j]; }\n"
             "  static constexpr bool prismatic(int j) { return kPri[j] != 0; }\n"
             "  static constexpr int last_child(int j) { int c = -1; for (int k = j + 1; k < N; ++k) if (kPar[k] == j) c = k; return c; }\n"
             "  static constexpr bool is_ancestor(int a, int i) { for (int k = kPar[i]; k >= 0; k = kPar[k]) if (k == a) return true; return false; }\n"
             "  static constexpr int child_toward(int a, int i) { int c = i; for (int k = kPar[i]; k >= 0; c = k, k = kPar[k]) if (k == a) return c; return -1; }\n"
             "  static constexpr bool on_path(int j) { return j == N - 1 || is_ancestor(j, N - 1); }\n"
             "};\n";
    }
    if (pack == 2 || pack == 4) {  // paired fp32 lanes: every constant splat to both halves (spatial.hip.hpp f2)
        o << "using TV = rbamd::dev::f2;\n";
        o << "static __device__ constexpr TV kModel[" << pk.size() << "] = {\n";
        for (size_t k = 0; k < pk.size(); ++k) {
            const std::string c = literal(pk[k], f64);
            o << "  TV{" << c << ", " << c << "},\n";
        }
    } else {
        o << "static __device__ constexpr T kModel[" << pk.size() << "] = {\n";
        for (size_t k = 0; k < pk.size(); ++k) o << "  " << literal(pk[k], f64) << ",\n";
    }
    o << "};\n";
    if (ext || lk || contact || rvjp || fvjp) {  // every link's axis frame R_a (model.cpp axis_frames): the identity for z-axis links
        const std::vector<double> ra = m.axis_frames();
        o << "static __device__ constexpr T kExtRa[" << ra.size() << "] = {\n";
        for (size_t k = 0; k < ra.size(); ++k) o << "  " << literal(snap(ra[k]), f64) << ",\n";
        o << "};\n";
    }
    if (contact) {
        // the contact set as compile-time constants: a point's link and position, the plane, the
        // law's parameters; kSlotOf[j] is link j's rank among the links that carry points (-1: none)
        const ContactSet &c = m.contacts;
        std::vector<int> slot_of(m.n, -1);
        int slots = 0;
        for (int j = 0; j < m.n; ++j)
            for (int p = 0; p < c.n_points; ++p)
                if (c.link[p] == j) {
                    slot_of[j] = slots++;
                    break;
                }
        o << "static __device__ constexpr int kConLink[" << c.n_points << "] = {";
        for (int p = 0; p < c.n_points; ++p) o << (p ? ", " : "") << c.link[p];
        o << "};\nstatic __device__ constexpr int kConSlotOf[N] = {";
        for (int j = 0; j < m.n; ++j) o << (j ? ", " : "") << slot_of[j];
        o << "};\nstatic __device__ constexpr T kConPoint[" << 3 * c.n_points << "] = {";
        for (int p = 0; p < c.n_points; ++p)
            for (int k = 0; k < 3; ++k) o << (p + k ? ", " : "") << literal(c.point[p][k], f64);
        o << "};\nstatic __device__ constexpr T kConNormal[3] = {" << literal(snap(c.normal[0]), f64) << ", "
          << literal(snap(c.normal[1]), f64) << ", " << literal(snap(c.normal[2]), f64) << "};\n";
        o << "struct Con {\n  static constexpr int kSlots = " << slots << ";\n"
          << "  static constexpr int points() { return " << c.n_points << "; }\n"
             "  static constexpr int link(int p) { return kConLink[p]; }\n"
             "  static constexpr int slot_of(int j) { return kConSlotOf[j]; }\n"
             "  static constexpr T point(int p, int k) { return kConPoint[3 * p + k]; }\n"
             "  static constexpr T normal(int k) { return kConNormal[k]; }\n"
          << "  static constexpr T offset() { return " << literal(c.offset, f64) << "; }\n"
          << "  static constexpr T stiffness() { return " << literal(c.stiffness, f64) << "; }\n"
          << "  static constexpr T damping() { return " << literal(c.damping, f64) << "; }\n"
          << "  static constexpr T friction() { return " << literal(c.friction, f64) << "; }\n"
          << "  static constexpr T slip_velocity() { return " << literal(c.slip_velocity, f64) << "; }\n};\n";
    }
    // ---- the kernel: one signature helper, one prologue per lane form
    const std::string head = std::string("extern \"C\" __global__ __launch_bounds__(256) ") +
                             (waves ? "__attribute__((amdgpu_waves_per_eu(" + std::to_string(waves) + "))) " : "") + "void ";
    auto sig = [&](const std::string &params) { o << head << "rb_jit_kernel(" << params << ") {\n"; };
    // Lane kernels take the block stride bs (elements): 256 for SoA, N * 256 for the tiled
    // layout (kernels.hpp); block k's arrays start at element k * bs, lane offset threadIdx.x.
    auto dyn_params = [](const char *in3, const char *out) {  // dynamics: three inputs, one output
        return std::string("const T *__restrict__ q, const T *__restrict__ qd, const T *__restrict__ ") + in3 +
               ", T *__restrict__ " + out + ", uint32_t B, int64_t ld, int64_t bs";
    };
    const char *fused_params =
        "const T *__restrict__ q, const T *__restrict__ qd, const T *__restrict__ qdd, const T *__restrict__ tau_in, "
        "T *__restrict__ tau, T *__restrict__ qdd_out, uint32_t B, int64_t ld, int64_t bs";
    const char *rollout_params =
        "T *__restrict__ q, T *__restrict__ qd, const T *__restrict__ tau_seq, T dt, int K, T *__restrict__ traj, "
        "uint32_t B, int64_t ld";
    // q-only kernels take the block strides of their input and output rows (256 for SoA;
    // n * 256 / rows * 256 for the tiled layout), as the lane kernels above
    auto q_params = [](const char *out) {
        return std::string("const T *__restrict__ q, T *__restrict__ ") + out +
               ", uint32_t B, int64_t ld, int64_t bs_in, int64_t bs_out";
    };
    // One configuration per lane: lane t of block k is configuration 256 k + t.
    const std::string lane_guard =
        "  const uint32_t b = blockIdx.x * 256u + threadIdx.x;\n"
        "  if (b >= B) return;\n";
    const std::string lane_prologue = lane_guard + "  const int64_t o = (int64_t)blockIdx.x * bs;\n";
    // Paired lanes: block k owns batch blocks 2k and 2k+1 (SoA: configurations 512k + t and
    // 512k + 256 + t; tiled: lane t of tiles 2k and 2k+1).  When the second is past B, the
    // lane evaluates the first twice and stores the bit-identical value twice.
    const char *pair_prologue =
        "  const uint32_t bA = blockIdx.x * 512u + threadIdx.x;\n"
        "  if (bA >= B) return;\n"
        "  const int64_t oA = (int64_t)(2u * blockIdx.x) * bs;\n"
        "  const uint32_t offA = threadIdx.x * 4u;\n"
        "  const uint32_t offB = bA + 256u < B ? offA + (uint32_t)bs * 4u : offA;\n";
    // Sequential pair (pack 3): lane t of batch blocks 2k and 2k+1, evaluated one after the
    // other from one load burst; the second only when it exists (twoB).
    const char *seq_prologue =
        "  const uint32_t bA = blockIdx.x * 512u + threadIdx.x;\n"
        "  if (bA >= B) return;\n"
        "  const int64_t oA = (int64_t)(2u * blockIdx.x) * bs;\n"
        "  const uint32_t offA = threadIdx.x * (uint32_t)sizeof(T);\n"
        "  const bool twoB = bA + 256u < B;\n"
        "  const uint32_t offB = offA + (uint32_t)bs * (uint32_t)sizeof(T);\n";
    if (kind == JitKind::Rnea) {
        sig(dyn_params("qdd", "tau"));
        const char *lane_args = "(kModel, q + o, qd + o, qdd + o, tau + o, threadIdx.x, ld);\n";
        if (pack == 3) {
            if (v.tail > 0) {
                // pairs of tiles for blocks < G1, then one tile per block for the last S tiles
                // (jit_grid below counts the same T_ / S_ / P_ / G1)
                o << "  const uint32_t T_ = (B + 255u) / 256u, S_ = (uint32_t)(((uint64_t)T_ * " << v.tail
                  << "u) / 100u);\n";
                o << "  const uint32_t P_ = (T_ - S_) & ~1u, G1 = P_ / 2u;\n";
                o << "  if (blockIdx.x >= G1) {\n";
                o << "    const uint32_t t = P_ + (blockIdx.x - G1), b = t * 256u + threadIdx.x;\n";
                o << "    if (b >= B) return;\n";
                o << "    const int64_t o = (int64_t)t * bs;\n";
                o << "    rbamd::dev::rnea_lane<T, N, " << F << ", Topo>" << lane_args << "    return;\n  }\n";
            }
            o << seq_prologue;
            o << "  rbamd::dev::rnea_lane_seq2<T, N, " << F
              << ", Topo>(kModel, q + oA, qd + oA, qdd + oA, tau + oA, offA, offB, twoB, ld);\n}\n";
        } else {
            o << lane_prologue;
            if (rev && com && pack == 1)
                o << "  rbamd::dev::rnea_lane_rev<T, N, " << F << ">";
            else if (park > 0)
                o << "  rbamd::dev::rnea_lane_park<T, N, " << F << ", " << park << ">";
            else
                o << "  rbamd::dev::rnea_lane<T, N, " << F << ", Topo>";
            o << lane_args << "}\n";
        }
    } else if (kind == JitKind::RneaFd) {
        // one configuration per lane; the launcher takes this kind only for mass-matrix models
        sig(fused_params);
        if (pack == 5) {
            o << "  rbamd::dev::idfd_split_block1<T, N, " << F << ">(kModel, q, qd, qdd, tau_in, tau, qdd_out, B, ld, bs);\n}\n";
        } else {
            o << lane_prologue;
            o << "  rbamd::dev::idfd_lane<T, N, " << F
              << ">(kModel, q + o, qd + o, qdd + o, tau_in + o, tau + o, qdd_out + o, threadIdx.x, ld);\n}\n";
        }
    } else if (kind == JitKind::Fd) {
        sig(dyn_params("tau", "qdd"));
        const char *lane_args = "(kModel, q + o, qd + o, tau + o, qdd + o, threadIdx.x, ld);\n}\n";
        const char *pair_args = "(kModel, q + oA, qd + oA, tau + oA, qdd + oA, offA, offB, ld);\n}\n";
        if (fdh && pack == 5) {
            o << "  rbamd::dev::fdh_split_block1<T, N, " << F << ">(kModel, q, qd, tau, qdd, B, ld, bs);\n}\n";
        } else if (fdh && pack == 4) {
            o << "  rbamd::dev::fdh_split_block2<N, " << F << ">(kModel, q, qd, tau, qdd, B, ld, bs);\n}\n";
        } else if (fdh && pack == 2) {
            o << pair_prologue << "  rbamd::dev::fdh_lane2<N, " << F << ">" << pair_args;
        } else if (fdh) {
            o << lane_prologue << "  rbamd::dev::fdh_lane<T, N, " << F << ", Topo>" << lane_args;
        } else if (pack == 3) {
            o << seq_prologue << "  rbamd::dev::aba_lane_seq2<T, N, " << F
              << ", Topo>(kModel, q + oA, qd + oA, tau + oA, qdd + oA, offA, offB, twoB, ld);\n}\n";
        } else if (pack == 2) {
            o << pair_prologue << "  rbamd::dev::aba_lane2<N, " << F << ", Topo>" << pair_args;
        } else {
            o << lane_prologue << "  rbamd::dev::aba_lane<T, N, " << F << ", Topo>" << lane_args;
        }
    } else if (ext) {
        // one configuration per lane on SoA rows; fext [6 N][ld] sits between the inputs and the output
        const bool fd = kind == JitKind::FdExt;
        sig(std::string("const T *__restrict__ q, const T *__restrict__ qd, const T *__restrict__ ") +
            (fd ? "tau" : "qdd") + ", const T *__restrict__ fext, T *__restrict__ " + (fd ? "qdd" : "tau") +
            ", uint32_t B, int64_t ld, int64_t bs");
        o << lane_prologue;
        if (fd)
            o << "  rbamd::dev::fd_ext_lane<T, N, " << F << ", Topo, " << (jit_fd_form(m) == 2 ? "true" : "false")
              << ">(kModel, kExtRa, q + o, qd + o, tau + o, fext + o, qdd + o, threadIdx.x, ld);\n}\n";
        else
            o << "  rbamd::dev::rnea_ext_lane<T, N, " << F
              << ", Topo>(kModel, kExtRa, q + o, qd + o, qdd + o, fext + o, tau + o, threadIdx.x, ld);\n}\n";
    } else if (rvjp) {
        // one configuration per lane on SoA rows; the plain form has no wrench parameters at all, the
        // wrench form takes fext and g_fext [6 N][ld]
        const bool wr = kind == JitKind::RneaVjpExt;
        sig(std::string("const T *__restrict__ q, const T *__restrict__ qd, const T *__restrict__ qdd, ") +
            (wr ? "const T *__restrict__ fext, " : "") +
            "const T *__restrict__ w, T *__restrict__ g_q, T *__restrict__ g_qd, T *__restrict__ g_qdd, " +
            (wr ? "T *__restrict__ g_fext, " : "") + "uint32_t B, int64_t ld, int64_t bs");
        o << lane_prologue << "  rbamd::dev::rnea_vjp_lane<T, N, " << F << ", Topo, " << (wr ? "true" : "false")
          << ">(kModel, kExtRa, q + o, qd + o, qdd + o, " << (wr ? "fext + o" : "nullptr")
          << ", w + o, g_q + o, g_qd + o, g_qdd + o, " << (wr ? "g_fext + o" : "nullptr")
          << ", threadIdx.x, ld);\n}\n";
    } else if (fvjp) {
        // one configuration per lane on SoA rows, as the inverse dynamics' gradient above; qdd is an output
        const bool wr = kind == JitKind::FdVjpExt;
        sig(std::string("const T *__restrict__ q, const T *__restrict__ qd, const T *__restrict__ tau, ") +
            (wr ? "const T *__restrict__ fext, " : "") +
            "const T *__restrict__ w, T *__restrict__ qdd, T *__restrict__ g_q, T *__restrict__ g_qd, "
            "T *__restrict__ g_tau, " + (wr ? "T *__restrict__ g_fext, " : "") + "uint32_t B, int64_t ld, int64_t bs");
        o << lane_prologue << "  rbamd::dev::fd_vjp_lane<T, N, " << F << ", Topo, " << (wr ? "true" : "false") << ", "
          << (jit_fd_form(m) == 2 ? "true" : "false") << ">(kModel, kExtRa, q + o, qd + o, tau + o, "
          << (wr ? "fext + o" : "nullptr") << ", w + o, qdd + o, g_q + o, g_qd + o, g_tau + o, "
          << (wr ? "g_fext + o" : "nullptr") << ", threadIdx.x, ld);\n}\n";
    } else if (kind == JitKind::ContactWrench) {
        // one configuration per lane on SoA rows: fext [6 N][ld], cforce [3 P][ld]
        sig("const T *__restrict__ q, const T *__restrict__ qd, T *__restrict__ fext, T *__restrict__ cforce, "
            "uint32_t B, int64_t ld, int64_t bs");
        o << lane_prologue << "  rbamd::dev::contact_wrench_lane<T, N, " << F
          << ", Topo, Con>(kModel, kExtRa, q + o, qd + o, fext + o, cforce + o, threadIdx.x, ld);\n}\n";
    } else if (kind == JitKind::RolloutContact) {
        sig(rollout_params);
        o << "  __shared__ rbamd::dev::RolloutShared<T, N> sh;\n";
        o << lane_guard;
        o << "  rbamd::dev::rollout_contact_lane<T, N, " << F << ", Topo, "
          << (jit_fd_form(m, JitKind::Rollout) == 2 ? "true" : "false")
          << ", Con>(kModel, kExtRa, q, qd, tau_seq, dt, K, traj, b, ld, sh);\n}\n";
    } else if (lk) {
        // one configuration per lane on SoA rows: pos [3 N][ld] and rot [9 N][ld], or vel [6 N][ld]
        if (kind == JitKind::LinkVel) {
            sig("const T *__restrict__ q, const T *__restrict__ qd, T *__restrict__ vel, uint32_t B, int64_t ld, int64_t bs");
            o << lane_prologue << "  rbamd::dev::link_vel_lane<T, N, " << F
              << ", Topo>(kModel, kExtRa, q + o, qd + o, vel + o, threadIdx.x, ld);\n}\n";
        } else {
            sig("const T *__restrict__ q, T *__restrict__ pos, T *__restrict__ rot, uint32_t B, int64_t ld, int64_t bs");
            o << lane_prologue << "  rbamd::dev::link_pose_lane<T, N, " << F
              << ", Topo>(kModel, kExtRa, q + o, pos + o, rot + o, threadIdx.x, ld);\n}\n";
        }
    } else if (cz) {
        // one configuration per lane on SoA rows: com [3][ld], hg [6][ld], energy [2][ld], ag [6 N][ld]
        if (kind == JitKind::Centroidal) {
            sig("const T *__restrict__ q, const T *__restrict__ qd, T *__restrict__ com, T *__restrict__ hg, "
                "T *__restrict__ energy, uint32_t B, int64_t ld, int64_t bs");
            o << lane_prologue << "  rbamd::dev::centroidal_lane<T, N, " << F
              << ", Topo>(kModel, q + o, qd + o, com + o, hg + o, energy + o, threadIdx.x, ld);\n}\n";
        } else {
            const bool cmm = kind == JitKind::Cmm;
            sig(std::string("const T *__restrict__ q, T *__restrict__ ") + (cmm ? "ag" : "com") +
                ", uint32_t B, int64_t ld, int64_t bs");
            o << lane_prologue << "  rbamd::dev::" << (cmm ? "cmm_lane" : "com_lane") << "<T, N, " << F
              << ", Topo>(kModel, q + o, " << (cmm ? "ag" : "com") << " + o, threadIdx.x, ld);\n}\n";
        }
    } else if (deriv) {
        // one configuration per lane on SoA rows; a NULL output is neither evaluated nor stored
        const bool fd = kind == JitKind::FdDeriv;
        sig(fd ? "const T *__restrict__ q, const T *__restrict__ qd, const T *__restrict__ tau, T *__restrict__ qdd, "
                 "T *__restrict__ dq, T *__restrict__ dqd, T *__restrict__ dtau, uint32_t B, int64_t ld, int64_t bs"
               : "const T *__restrict__ q, const T *__restrict__ qd, const T *__restrict__ qdd, T *__restrict__ dq, "
                 "T *__restrict__ dqd, uint32_t B, int64_t ld, int64_t bs");
        o << lane_prologue;
        if (fd)
            o << "  rbamd::dev::fd_deriv_lane<T, N, " << F
              << ">(kModel, q + o, qd + o, tau + o, qdd ? qdd + o : nullptr, dq ? dq + o : nullptr, "
                 "dqd ? dqd + o : nullptr, dtau ? dtau + o : nullptr, threadIdx.x, ld);\n}\n";
        else
            o << "  rbamd::dev::rnea_deriv_lane<T, N, " << F
              << ">(kModel, q + o, qd + o, qdd + o, dq ? dq + o : nullptr, dqd ? dqd + o : nullptr, threadIdx.x, ld);\n}\n";
    } else if (vjp) {
        // one configuration per lane on SoA rows, K steps forward then K back (rollout_vjp_body.hip.hpp,
        // contact_vjp_body.hip.hpp)
        sig("const T *__restrict__ q, const T *__restrict__ qd, const T *__restrict__ tau_seq, T dt, int K, "
            "const T *__restrict__ gq, const T *__restrict__ gqd, T *__restrict__ g_q0, T *__restrict__ g_qd0, "
            "T *__restrict__ g_tau, T *work, uint32_t B, int64_t ld");
        o << lane_guard;
        if (cvjp)
            o << "  rbamd::dev::rollout_contact_vjp_lane<T, N, " << F
              << ", Topo, Con>(kModel, kExtRa, q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau, work, b, ld);\n}\n";
        else
            o << "  rbamd::dev::rollout_vjp_lane<T, N, " << F
              << ">(kModel, q, qd, tau_seq, dt, K, gq, gqd, g_q0, g_qd0, g_tau, work, b, ld);\n}\n";
    } else if (kind == JitKind::Rollout) {
        sig(rollout_params);
        if (pack == 4) {
            o << "  rbamd::dev::rollout_split_block2<N, " << F << ">(kModel, q, qd, tau_seq, dt, K, traj, B, ld);\n}\n";
        } else if (pack == 2) {
            o << "  __shared__ rbamd::dev::RolloutShared2<N> sh;\n";
            o << "  const uint32_t bA = blockIdx.x * 512u + threadIdx.x;\n";
            o << "  if (bA >= B) return;\n";
            o << "  const uint32_t offA = bA * 4u, offB = bA + 256u < B ? offA + 1024u : offA;\n";
            o << "  rbamd::dev::rollout_lane2<N, " << F << ", Topo>(kModel, q, qd, tau_seq, dt, K, traj, offA, offB, ld, sh);\n}\n";
        } else {
            o << "  __shared__ rbamd::dev::RolloutShared<T, N> sh;\n";
            o << lane_guard;
            o << "  rbamd::dev::rollout_lane<T, N, " << F << ", Topo>(kModel, q, qd, tau_seq, dt, K, traj, b, ld, sh);\n}\n";
        }
    } else {  // CRBA, fwd_kin, jac
        const char *out = kind == JitKind::Crba ? "H" : "out";
        const char *lane = kind == JitKind::Crba ? "crba_lane" : kind == JitKind::FwdKin ? "fwd_kin_lane_tree" : "jac_lane_tree";
        sig(q_params(out));
        o << lane_guard;
        o << "  rbamd::dev::" << lane << "<T, N, " << F << ", Topo>(kModel, q + (int64_t)blockIdx.x * bs_in, " << out
          << " + (int64_t)blockIdx.x * bs_out, threadIdx.x, ld);\n}\n";
    }
    std::string src = o.str();
    if (tab) {  // every kernel fills the block's sincos table first (all lanes still present)
        const size_t at = src.find("rb_jit_kernel(");
        const size_t body = at == std::string::npos ? at : src.find(") {\n", at);
        if (body != std::string::npos) src.insert(body + 4, "  rbamd::dev::sctab_init();\n");
    }
    return src;
}

unsigned jit_grid(const JitKernel &jk, uint32_t B) {
    const int pack = jk.variant.pack;
    if (pack == 3 && jk.variant.tail > 0) {  // pairs, then a one-per-lane tail (jit_source's T_ / S_ / P_ / G1)
        const unsigned T = (unsigned)(((uint64_t)B + 255u) / 256u);
        const unsigned S = (unsigned)(((uint64_t)T * (unsigned)jk.variant.tail) / 100u);
        const unsigned P = (T - S) & ~1u;
        return P / 2u + (T - P);
    }
    // pack 2 / 3: two configurations per lane; pack 5: the one-per-lane wave split, 128 per block
    // (pack 4, the packed split, covers 256 per block like one per lane)
    const unsigned per_block = pack == 5 ? 128u : 256u * ((pack == 2 || pack == 3) ? 2u : 1u);
    return (unsigned)(((uint64_t)B + per_block - 1) / per_block);
}

namespace {
bool rtc_compile(const std::string &src, const std::string &arch, bool no_licm, bool no_slp, std::vector<char> *code,
                 std::string *error) {
    hiprtcProgram prog = nullptr;
    if (hiprtcCreateProgram(&prog, src.c_str(), "rb_jit.hip", kJitHeaderCount, kJitHeaderSources,
                            kJitHeaderNames) != HIPRTC_SUCCESS) {
        *error = "hiprtcCreateProgram failed";
        return false;
    }
    const std::string arch_opt = "--offload-arch=" + arch;
    const char *opts[] = {arch_opt.c_str(), "-O3", "-std=c++17", "-ffinite-math-only", "-fno-signed-zeros"};
    std::vector<const char *> optv(opts, opts + sizeof(opts) / sizeof(opts[0]));
    if (no_licm) {
        optv.push_back("-mllvm");
        optv.push_back("-disable-machine-licm");
    }
    if (no_slp) optv.push_back("-fno-slp-vectorize");
    const int preload = tuning().kernarg_preload;
    const std::string preload_opt = "-amdgpu-kernarg-preload-count=" + std::to_string(preload);
    if (preload > 0) {
        optv.push_back("-mllvm");
        optv.push_back(preload_opt.c_str());
    }
    hiprtcResult rc = hiprtcCompileProgram(prog, (int)optv.size(), optv.data());
    if (rc != HIPRTC_SUCCESS) {
        size_t n = 0;
        hiprtcGetProgramLogSize(prog, &n);
        std::string log(n, '\0');
        if (n) hiprtcGetProgramLog(prog, &log[0]);
        *error = std::string("hiprtc compile failed: ") + hiprtcGetErrorString(rc) + "\n" + log;
        hiprtcDestroyProgram(&prog);
        return false;
    }
    size_t code_size = 0;
    hiprtcGetCodeSize(prog, &code_size);
    code->resize(code_size);
    hiprtcGetCode(prog, code->data());
    hiprtcDestroyProgram(&prog);
    return true;
}
}  // namespace

bool jit_compile(const Model &m, const JitVariant &v, const std::string &arch, std::vector<char> *code,
                 std::string *error, std::string *final_src) {
    const std::string why = jit_kind_unsupported(m, v.kind);
    if (!why.empty()) {
        *error = why;
        return false;
    }
    std::string src = jit_source(m, v, -1);
    const bool no_licm = jit_no_licm(m, v);
    const bool no_slp = jit_no_slp(v);
    if (!rtc_compile(src, arch, no_licm, no_slp, code, error)) return false;
    // Occupancy cliff (jit.hpp): no target asked for, none in the source, and the kernel just
    // past 256 registers -> rebuild with a 2-wave target; the first build stands if that fails.
    if (tuning().jit_waves < 0 && src.find("amdgpu_waves_per_eu") == std::string::npos) {
        const int vgprs = code_vgprs(*code);
        if (vgprs > 256 && vgprs <= 272) {
            std::string src2 = jit_source(m, v, 2), err2;
            std::vector<char> code2;
            if (rtc_compile(src2, arch, no_licm, no_slp, &code2, &err2)) {
                code->swap(code2);
                src.swap(src2);
            }
        }
    }
    if (final_src) *final_src = src;
    // RB_JIT_DUMP=dir: keep every compiled source and code object for inspection
    // (llvm-objdump / llvm-readelf on the .co: registers, scratch, ISA of what really runs)
    if (const char *dir = std::getenv("RB_JIT_DUMP")) {
        static std::atomic<int> seq{0};
        const std::string base = std::string(dir) + "/jit_" + std::to_string(seq.fetch_add(1)) + "_k" +
                                 std::to_string((int)v.kind) + (v.f64 ? "_f64" : "_f32") + "_p" + std::to_string(v.pack);
        if (FILE *f = std::fopen((base + ".hip").c_str(), "wb")) {
            std::fwrite(src.data(), 1, src.size(), f);
            std::fclose(f);
        }
        if (FILE *f = std::fopen((base + ".co").c_str(), "wb")) {
            std::fwrite(code->data(), 1, code->size(), f);
            std::fclose(f);
        }
    }
    return true;
}

JitKernel jit_build(const Model &m, const JitVariant &v) {
    JitKernel jk;
    jk.variant = v;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        jk.error = "no HIP device";
        return jk;
    }
    std::vector<char> code;
    if (!jit_compile(m, v, prop.gcnArchName, &code, &jk.error)) return jk;
    hipError_t e = hipModuleLoadData(&jk.module, code.data());
    if (e != hipSuccess) {
        jk.error = std::string("hipModuleLoadData: ") + hipGetErrorString(e);
        jk.module = nullptr;
        return jk;
    }
    e = hipModuleGetFunction(&jk.function, jk.module, "rb_jit_kernel");
    if (e != hipSuccess) {
        jk.error = std::string("hipModuleGetFunction: ") + hipGetErrorString(e);
        (void)hipModuleUnload(jk.module);
        jk.module = nullptr;
        jk.function = nullptr;
        return jk;
    }
    return jk;
}

}  // namespace rbamd
