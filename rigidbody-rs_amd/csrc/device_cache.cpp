// device_cache.cpp -- per-handle device state (device_cache.hpp).
#include "device_cache.hpp"

#include "tuning.hpp"

namespace rbamd {

template <typename T>
hipError_t DeviceCache::consts_of(const std::vector<T> &host, T *Consts::*block, const T **out, const char **where) {
    int d = 0;
    hipError_t e = hipGetDevice(&d);
    *where = "hipGetDevice";
    if (e != hipSuccess) return e;
    std::atomic<const void *> *fastp = (d >= 0 && d < kDevices) ? &consts_fast_[d][sizeof(T) == 8 ? 1 : 0] : nullptr;
    if (fastp) {
        if (const void *p = fastp->load(std::memory_order_acquire)) {
            *out = static_cast<const T *>(p);
            return hipSuccess;
        }
    }
    std::lock_guard<std::mutex> lk(mu_);
    T *&dev = consts_[d].*block;
    if (!dev) {
        void *p = nullptr;
        const size_t bytes = host.size() * sizeof(T);
        *where = "hipMalloc(model)";
        if ((e = hipMalloc(&p, bytes)) != hipSuccess) return e;
        *where = "hipMemcpy(model)";
        if ((e = hipMemcpy(p, host.data(), bytes, hipMemcpyHostToDevice)) != hipSuccess) {
            (void)hipFree(p);
            return e;
        }
        dev = static_cast<T *>(p);
    }
    *out = dev;
    if (fastp) fastp->store(dev, std::memory_order_release);
    return hipSuccess;
}

hipError_t DeviceCache::consts(const std::vector<float> &host, const float **out, const char **where) {
    return consts_of<float>(host, &Consts::f32, out, where);
}
hipError_t DeviceCache::consts(const std::vector<double> &host, const double **out, const char **where) {
    return consts_of<double>(host, &Consts::f64, out, where);
}

const JitKernel *DeviceCache::kernel(const Model &m, const JitVariant &v) {
    if (!jit_enabled()) return nullptr;
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) return nullptr;
    std::atomic<const Pub *> *slot = nullptr;
    if (d >= 0 && d < kDevices && (int)v.kind >= 0 && (int)v.kind < kJitKinds && v.pack >= 0 && v.pack < 6) {
        slot = &jit_fast_[d][(int)v.kind][v.f64 ? 1 : 0][v.fast ? 1 : 0][v.pack][(v.tail > 0 ? 1 : 0) | (v.nt >= 0 ? 2 : 0)];
        if (const Pub *p = slot->load(std::memory_order_acquire))
            if (p->gen.load(std::memory_order_acquire) == tuning_generation()) return p->jk;
    }
    std::lock_guard<std::mutex> lk(mu_);
    // The tuning generation is a sequence count (tuning.cpp): odd while rb_set_tuning writes,
    // bumped again after.  The key and the kernel source both read the tuning knobs, so they are
    // resolved between two reads of one even generation; a write in between resolves again (a
    // kernel built from a mix of two tunings is never stored under either key).
    for (;;) {
        const unsigned gen = tuning_generation_stable();
        const std::string key = std::to_string(d) + jit_key(m, v);
        auto it = jit_.find(key);
        if (it == jit_.end()) {
            JitKernel built = jit_build(m, v);
            if (tuning_generation() != gen) {  // the tuning moved under the build
                if (built.module) (void)hipModuleUnload(built.module);
                continue;
            }
            it = jit_.emplace(key, Entry{std::move(built), d}).first;
        }
        const JitKernel *res = it->second.jk.function ? &it->second.jk : nullptr;
        if (tuning_generation() != gen) continue;
        if (slot && res) {
            // jk is written once, when the record is created (the key holds the same pointer), and
            // never again: fast-path readers may hold the record while this re-stamps gen
            auto ins = pub_.try_emplace({(const void *)slot, res});
            Pub &rec = ins.first->second;
            if (ins.second) rec.jk = res;
            rec.gen.store(gen, std::memory_order_release);
            slot->store(&rec, std::memory_order_release);
        }
        return res;
    }
}

std::vector<std::string> DeviceCache::jit_errors() {
    std::vector<std::string> out;
    std::lock_guard<std::mutex> lk(mu_);
    for (auto &kv : jit_)
        if (!kv.second.jk.error.empty()) out.push_back(kv.second.jk.error);
    return out;
}

DeviceCache::~DeviceCache() {
    std::lock_guard<std::mutex> lk(mu_);
    int cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    for (auto &kv : consts_) {
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        if (kv.second.f32) (void)hipFree(kv.second.f32);
        if (kv.second.f64) (void)hipFree(kv.second.f64);
    }
    for (auto &kv : jit_) {
        if (!kv.second.jk.module) continue;
        if (hipSetDevice(kv.second.device) != hipSuccess) continue;
        (void)hipModuleUnload(kv.second.jk.module);
    }
    if (have_cur) (void)hipSetDevice(cur);
}

}  // namespace rbamd
