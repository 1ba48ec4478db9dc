// The host side of a satellite library's C ABI: the error text behind <prefix>_last_error(), the two ways an entry point fails, the
// launch check and the grid size.  Every definition is inline in a namespace of hidden visibility: the translation units of one
// library share one buffer per thread, nothing is exported, and two libraries in one process never share theirs.
// libonepose_hip.so keeps its own (api.hip, tile.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

namespace capi __attribute__((visibility("hidden"))) {

inline thread_local char g_error[256] = "";

inline int fail(hipError_t e, const char* where) {          // a positive HIP error code
    snprintf(g_error, sizeof g_error, "%s: %s", where, hipGetErrorString(e));
    return (int)e > 0 ? (int)e : 1;
}

inline int bad_arg(const char* where, const char* what) {   // -1
    snprintf(g_error, sizeof g_error, "%s: %s", where, what);
    return -1;
}

inline unsigned blocks_of(long long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace capi

#define CAPI_CHECK_LAUNCH()                                       \
    do {                                                          \
        hipError_t e__ = hipGetLastError();                       \
        if (e__ != hipSuccess) return capi::fail(e__, __func__);  \
    } while (0)
