// device_cache.hpp -- what one Multibody handle keeps on the devices it has run on: the packed
// model constants (one upload per device and dtype) and the model-specialised hipRTC kernels
// (one build per jit_key).  Both are filled under one lock and read without it on a hit.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "jit.hpp"
#include "model.hpp"

namespace rbamd {

class DeviceCache {
public:
    DeviceCache() = default;
    DeviceCache(const DeviceCache &) = delete;
    DeviceCache &operator=(const DeviceCache &) = delete;
    // Frees the constants and unloads the modules, each on its own device; the caller's current
    // device is restored.  No call may be in flight on the handle.
    ~DeviceCache();

    // Device copy of `host` (the model's packed fp32 / fp64 constants) on the current device,
    // uploaded on first use.  On failure *where names the HIP call that failed.
    hipError_t consts(const std::vector<float> &host, const float **out, const char **where);
    hipError_t consts(const std::vector<double> &host, const double **out, const char **where);

    // The hipRTC kernel of variant `v` (jit.hpp jit_resolve) of model `m` on the current device,
    // built on first use; nullptr when hipRTC is disabled or the build failed.
    const JitKernel *kernel(const Model &m, const JitVariant &v);

    // The hipRTC logs of the builds that failed, in key order.
    std::vector<std::string> jit_errors();

private:
    struct Consts {
        float *f32 = nullptr;
        double *f64 = nullptr;
    };
    struct Entry {
        JitKernel jk;
        int device = 0;
    };
    // kernel()'s per-launch fast path: [device][kind][f64][fast trig][pack][tail, nt] of the
    // variant -> the kernel resolved under one tuning generation, published as ONE pointer to a
    // record {generation, kernel}.  There is one record per (slot, kernel) pair, so the records are
    // bounded by slots x kernels however often the tuning changes: a record's kernel never
    // changes, its generation is re-stamped only when ITS slot resolves to that kernel again,
    // and records live in pub_ (std::map nodes never move) until the cache dies.  A reader that sees
    // the current generation in the record its slot points at has that slot's kernel.
    struct Pub {
        std::atomic<unsigned> gen{0};
        const JitKernel *jk = nullptr;
    };
    static constexpr int kDevices = 16;  // devices with a lock-free path; others take the lock

    template <typename T>
    hipError_t consts_of(const std::vector<T> &host, T *Consts::*block, const T **out, const char **where);

    std::mutex mu_;
    std::map<int, Consts> consts_;
    std::map<std::string, Entry> jit_;  // keyed by device + jit_key (kind, dtype, trig, tuning tag, form)
    std::map<std::pair<const void *, const JitKernel *>, Pub> pub_;
    std::atomic<const Pub *> jit_fast_[kDevices][kJitKinds][2][2][6][4] = {};  // last: tail > 0, nt override
    std::atomic<const void *> consts_fast_[kDevices][2] = {};                  // set once, never moved
};

}  // namespace rbamd
