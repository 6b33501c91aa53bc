// The host plumbing every context-free library (libbusca_track.so ... libbusca_mgframe.so) shares: the thread's error message, the refusal that records
// it, the alignment test, the device scope and the launch macros.  Included once by the library's one translation unit, after its kernels and after
//     #define CAPI_EHIP   BUSCA_<STEM>_EHIP        (what a failed HIP call returns)
//     #define CAPI_EINVAL BUSCA_<STEM>_EINVAL      (only with CAPI_STORE_ARGS)
// Everything is static: each library keeps its own g_err.  Not for libbusca_hip.so, whose errors belong to its context (busca_internal.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#ifndef CAPI_EHIP
#error "define CAPI_EHIP (the library's BUSCA_<STEM>_EHIP) before including capi_prelude.hpp"
#endif

static thread_local char g_err[320] = "";

static int refuse(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

static inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// `device` current for one launch, the previous one back afterwards
struct DeviceScope {
    int prev = -1;
    hipError_t err;
    explicit DeviceScope(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) err = hipSetDevice(device);
        else if (err == hipSuccess) prev = -1;
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// `device` current to the end of the enclosing block: for a call that launches more than once, or sets a kernel attribute first
#define CAPI_SCOPE(who, device)                                                                                         \
    DeviceScope scope(device);                                                                                          \
    if (scope.err != hipSuccess) return refuse(CAPI_EHIP, "%s: %s", who, hipGetErrorString(scope.err))

// one launch inside a CAPI_SCOPE, with `lds` bytes of dynamic LDS
#define CAPI_LAUNCH_IN_SCOPE(who, kernel, grid, block, lds, stream, ...)                                                \
    do {                                                                                                                \
        hipLaunchKernelGGL(kernel, grid, block, lds, (hipStream_t)(stream), __VA_ARGS__);                               \
        const hipError_t e_ = hipGetLastError();                                                                        \
        if (e_ != hipSuccess) return refuse(CAPI_EHIP, "%s: %s", who, hipGetErrorString(e_));                           \
    } while (0)

// the scope and one launch without dynamic LDS: what a call of one kernel needs
#define CAPI_LAUNCH(who, device, kernel, grid, block, stream, ...)                                                      \
    do {                                                                                                                \
        CAPI_SCOPE(who, device);                                                                                        \
        CAPI_LAUNCH_IN_SCOPE(who, kernel, grid, block, 0, stream, __VA_ARGS__);                                         \
    } while (0)

#ifdef CAPI_STORE_ARGS
// the checks every call makes of a Kalman store and its slot list -> 0, or the refusal already recorded.  `cov_needed`: some calls read the means alone.
static int store_args(const char* who, const double* mean, const double* cov, bool cov_needed, int32_t S, const int32_t* slot, int32_t n, int32_t device) {
    if (S < 0 || n < 0) return refuse(CAPI_EINVAL, "%s: negative size (S %d, n %d)", who, S, n);
    if (device < 0) return refuse(CAPI_EINVAL, "%s: negative device %d", who, device);
    if (n == 0) return 0;
    if (!mean || (cov_needed && !cov) || !slot) return refuse(CAPI_EINVAL, "%s: null pointer (mean, cov and slot are required)", who);
    if (misaligned(mean, 8) || misaligned(cov, 8) || misaligned(slot, 4))
        return refuse(CAPI_EINVAL, "%s: misaligned pointer (8 bytes for float64, 4 for int32)", who);
    return 0;
}
#endif
