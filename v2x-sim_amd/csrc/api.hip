// ABI version + per-thread error text of libv2x_amd.so (see include/v2x_amd.h).
#include "common.h"
#include <cxxabi.h>
#include <dlfcn.h>
#include <stdlib.h>
#include <string.h>

static thread_local char g_err[512] = "";

void v2x_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// A library that contains an INSTRUMENTED kernel object (tools/probes/*.patch built with a -DV2X_*_DBG_BUILD flag: phase-removal switches, time stamps -- its results are
// garbage) defines v2x_probe_build_marker; the version then reads NEGATIVE, which every loader that checks it refuses (v2x_sim_amd/_lib.py: unless V2X_ALLOW_PROBE_BUILD=1).
extern "C" __attribute__((weak)) int v2x_probe_build_marker;
extern "C" int v2x_abi_version(void) { return &v2x_probe_build_marker != nullptr ? -V2X_AMD_ABI_VERSION : V2X_AMD_ABI_VERSION; }

// ---- plan mode of v2x_launch (common.h) -------------------------------------------------------------------------------------------
struct v2x_launch_plan { char *buf; size_t cap, len; };
__thread v2x_launch_plan *v2x_plan_sink = nullptr;

// Appends the kernel's name as a profiler prints it: the host-side handle of a __global__ function carries the kernel's own mangled name, so the
// name comes from the pointer that would have been launched.  Demangled, then the leading "void " and the closing argument list cut away.
int v2x_plan_record(const void *kernel, const char *what) {
    v2x_launch_plan &p = *v2x_plan_sink;
    Dl_info info;
    char *dem = nullptr;
    if (dladdr(kernel, &info) != 0 && info.dli_sname && info.dli_saddr == kernel) dem = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, nullptr);
    if (!dem) {
        v2x_set_error("%s: the kernel's symbol does not resolve (plan mode needs kernels with external linkage)", what);
        return V2X_EIO;
    }
    const char *b = strncmp(dem, "void ", 5) == 0 ? dem + 5 : dem;
    size_t n = strlen(b);
    if (n > 0 && b[n - 1] == ')') {
        int depth = 0;
        for (size_t i = n; i-- > 0;) {
            if (b[i] == ')') ++depth;
            else if (b[i] == '(' && --depth == 0) { n = i; break; }
        }
    }
    const size_t sep = p.len ? 3 : 0;
    const bool fits = p.len + sep + n + 1 <= p.cap;
    if (fits) {
        memcpy(p.buf + p.len, " + ", sep);
        memcpy(p.buf + p.len + sep, b, n);
        p.len += sep + n;
        p.buf[p.len] = 0;
    }
    free(dem);
    V2X_REQUIRE(fits, "v2x_conv2d_plan: the kernel names do not fit %zu bytes", p.cap);
    return V2X_OK;
}

extern "C" int v2x_conv2d_plan(const v2x_conv_desc *d, char *buf, size_t cap) {
    V2X_REQUIRE(buf && cap > 0, "v2x_conv2d_plan: no buffer");
    buf[0] = 0;
    v2x_launch_plan plan = {buf, cap, 0};
    v2x_plan_sink = &plan;
    const int rc = v2x_conv2d(d, nullptr);
    v2x_plan_sink = nullptr;
    return rc;
}

// ---- tuning switches (common.h: v2x_tune_id) -----------------------------------------------------------------------------------
#include <atomic>
#include <mutex>
#include <strings.h>
namespace {
struct TuneEntry { const char *name; int def; };
const TuneEntry kTune[V2X_TUNE_COUNT] = {
    {"STREAM_WAVES", 8}, {"STREAM_G", 1}, {"STREAM_WT", 1}, {"STORE_X4", 1}, {"STREAM_PERSIST", 1}, {"STREAM_WIDE", 1},
    {"WIDE3", 1}, {"HALO_PP", 1}, {"VOXELIZE_LDS", 1}, {"WARP_LDS", 2}, {"S2_G", 1}, {"GRU_XCD_WALK", 1}, {"HALO_XCD", 1}, {"WGRAD_TR", 1}, {"BN_PARTIAL_T", 1}, {"WGRAD_REDUCE4", 1}, {"CONV1X1", 1},
};
std::atomic<int> g_tune[V2X_TUNE_COUNT];
std::once_flag g_tune_once;
void tune_init() {
    for (int i = 0; i < V2X_TUNE_COUNT; ++i) {
        char env[64];
        snprintf(env, sizeof(env), "V2X_%s", kTune[i].name);
        const char *e = getenv(env);                       // the ONLY getenv of the library, once per process
        g_tune[i].store((e && *e) ? atoi(e) : kTune[i].def, std::memory_order_relaxed);
    }
}
int tune_find(const char *name) {
    if (!name) return -1;
    if (strncasecmp(name, "V2X_", 4) == 0) name += 4;
    for (int i = 0; i < V2X_TUNE_COUNT; ++i)
        if (strcasecmp(name, kTune[i].name) == 0) return i;
    return -1;
}
}  // namespace

int v2x_tune(int id) {
    std::call_once(g_tune_once, tune_init);
    return g_tune[id].load(std::memory_order_relaxed);
}
extern "C" int v2x_tuning_set(const char *name, int value) {
    const int i = tune_find(name);
    V2X_REQUIRE(i >= 0, "v2x_tuning_set: unknown switch '%s'", name ? name : "(null)");
    std::call_once(g_tune_once, tune_init);
    g_tune[i].store(value, std::memory_order_relaxed);
    return V2X_OK;
}
extern "C" int v2x_tuning_get(const char *name, int *value) {
    const int i = tune_find(name);
    V2X_REQUIRE(i >= 0 && value, "v2x_tuning_get: unknown switch '%s' or null result", name ? name : "(null)");
    *value = v2x_tune(i);
    return V2X_OK;
}
extern "C" const char *v2x_last_error(void) { return g_err; }
