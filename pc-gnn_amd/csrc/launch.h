// Host-side launch bookkeeping, one copy for the whole library: the opt-in to more than 64 KiB of dynamic LDS and the device's CU
// count, both kept per device under one mutex.  The functions are `inline` with external linkage, so every translation unit that
// includes this header shares the one launch_cache() the linker keeps - there is no cache per .hip file.
#pragma once
#include <map>
#include <mutex>
#include <set>
#include <utility>

#include "common.h"

namespace pcg {

struct LaunchCache {
    std::mutex lock;
    std::set<std::pair<const void *, int>> lds_allowed;   // (kernel, device) pairs whose attribute is set
    std::map<int, int> cus;                               // device -> compute units
};
inline LaunchCache &launch_cache() {
    static LaunchCache c;
    return c;
}

// Let `kernel` be launched with up to `bytes` of dynamic LDS on the current device: the attribute is set once per kernel and
// device (it belongs to a device's copy of the kernel), whichever host thread comes first.  PCG_OK or PCG_E_LAUNCH.
inline int allow_dynamic_lds(const void *kernel, int bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return PCG_E_LAUNCH;
    LaunchCache &c = launch_cache();
    std::lock_guard<std::mutex> hold(c.lock);
    if (c.lds_allowed.count({kernel, dev})) return PCG_OK;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return PCG_E_LAUNCH;
    c.lds_allowed.insert({kernel, dev});
    return PCG_OK;
}
template <class... Args>
inline int allow_dynamic_lds(void (*kernel)(Args...), int bytes) {
    return allow_dynamic_lds(reinterpret_cast<const void *>(kernel), bytes);
}

// compute units of the current device, or `otherwise` when the query fails (a failure is not remembered)
inline int device_cus(int otherwise) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return otherwise;
    LaunchCache &c = launch_cache();
    std::lock_guard<std::mutex> hold(c.lock);
    const auto known = c.cus.find(dev);
    if (known != c.cus.end()) return known->second;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) return otherwise;
    c.cus[dev] = n;
    return n;
}

}  // namespace pcg
