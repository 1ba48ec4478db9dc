// What the two source files of libonepose_track.so share: the error text behind optrk_last_error().
#pragma once
#include <hip/hip_runtime.h>

namespace optrk {

int fail(hipError_t e, const char* where);              // a positive HIP error code
int bad_arg(const char* where, const char* what);       // -1

}  // namespace optrk

#define OPTRK_CHECK_LAUNCH()                                      \
    do {                                                          \
        hipError_t e__ = hipGetLastError();                       \
        if (e__ != hipSuccess) return optrk::fail(e__, __func__); \
    } while (0)
