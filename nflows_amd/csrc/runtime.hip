// The library's process state and host utilities (no kernels): the last HIP error, the CU count, the opt-in to more
// than 64 KB of dynamic LDS, the label of the last layer kernel, the measurement aid's event pool, and the ABI's
// version / error strings.  Declared in common.hpp, used by every launcher.

#include "common.hpp"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <set>
#include <utility>
#include <vector>

namespace nfa {

static thread_local int g_last_hip_error = 0;

int set_hip_error(hipError_t e) {
    g_last_hip_error = (int)e;
    return NFA_ERR_HIP;
}

int device_cu_count() {
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cached[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        cached[dev] = n;
    }
    return cached[dev];
}

// ---- optional measurement aid (bench.py): per-launch begin/end timestamps of the layer kernels.
// launch_kernel (common.hpp) attaches a start and a stop event to the dispatch itself, so
// hipEventElapsedTime(start, stop) is the kernel's own duration on its stream (what rocprofv3's
// kernel trace reports), free of launch gaps.  Off by default.
struct ProfileState {
    std::mutex mu;
    bool enabled = false;
    size_t capacity = 0;
    std::vector<hipEvent_t> start, stop;
};
static ProfileState g_profile;

// Hands out a start/stop event pair for the next profiled launch (null when profiling is off or
// the budget is used up).  Shared with the other translation units through common.hpp.
void profile_next_launch(hipEvent_t* start, hipEvent_t* stop) {
    *start = *stop = nullptr;
    std::lock_guard<std::mutex> lock(g_profile.mu);
    if (g_profile.enabled && g_profile.start.size() < g_profile.capacity) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
            g_profile.start.push_back(e0);
            g_profile.stop.push_back(e1);
            *start = e0;
            *stop = e1;
        }
    }
}

static thread_local char g_last_layer_kernel[192] = "";

void note_layer_kernel(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_layer_kernel, sizeof(g_last_layer_kernel), fmt, ap);
    va_end(ap);
}

int raise_dynamic_lds(const void* kern, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> raised;   // (kernel, device) pairs already opted in
    int dev = 0;
    NFA_HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    if (raised.count({kern, dev})) return NFA_OK;
    NFA_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    raised.insert({kern, dev});
    return NFA_OK;
}

}  // namespace nfa

using namespace nfa;

extern "C" int nfa_abi_version(void) { return NFA_ABI_VERSION; }
extern "C" const char* nfa_build_arch(void) { return "gfx950"; }
extern "C" int nfa_last_hip_error(void) { return g_last_hip_error; }
extern "C" const char* nfa_strerror(int code) {
    switch (code) {
        case NFA_OK: return "ok";
        case NFA_ERR_INVALID_ARGUMENT: return "invalid argument";
        case NFA_ERR_UNSUPPORTED: return "unsupported configuration for the fused kernel";
        case NFA_ERR_MIN_BIN_WIDTH: return "Minimal bin width too large for the number of bins";
        case NFA_ERR_MIN_BIN_HEIGHT: return "Minimal bin height too large for the number of bins";
        case NFA_ERR_HIP: return "HIP runtime error";
        default: return "unknown error";
    }
}

extern "C" int nfa_last_layer_kernel(char* buffer, int32_t capacity) {
    if (capacity < 0 || (capacity > 0 && !buffer)) return NFA_ERR_INVALID_ARGUMENT;
    if (capacity > 0) snprintf(buffer, (size_t)capacity, "%s", g_last_layer_kernel);
    return (int)strlen(g_last_layer_kernel);
}

extern "C" int nfa_profile_enable(int32_t max_launches) {
    if (max_launches < 0) return NFA_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(g_profile.mu);
    g_profile.enabled = max_launches > 0;
    g_profile.capacity = (size_t)max_launches;
    return NFA_OK;
}

extern "C" int nfa_profile_collect(float* durations_ms, int32_t capacity, int32_t* count) {
    if (!count || capacity < 0 || (capacity > 0 && !durations_ms)) return NFA_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lock(g_profile.mu);
    int32_t n = 0;
    for (size_t i = 0; i < g_profile.start.size(); ++i) {
        NFA_HIP_CHECK(hipEventSynchronize(g_profile.stop[i]));
        float ms = 0.0f;
        NFA_HIP_CHECK(hipEventElapsedTime(&ms, g_profile.start[i], g_profile.stop[i]));
        if (n < capacity) durations_ms[n++] = ms;
        (void)hipEventDestroy(g_profile.start[i]);
        (void)hipEventDestroy(g_profile.stop[i]);
    }
    g_profile.start.clear();
    g_profile.stop.clear();
    *count = n;
    return NFA_OK;
}
