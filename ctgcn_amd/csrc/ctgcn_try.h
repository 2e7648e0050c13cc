// ctgcn_try.h — host-side error plumbing shared by every kernel file: the thread-local error setter of ctgcn_hip.hip, the macro that
// turns a failed HIP call into CTGCN_E_HIP with the message "<expr> -> <hip error string>", the refusal "<what>: <text>" of an argument
// check, the alignment tests behind every float4 path, and the opt-in to more than 64 KiB of LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/ctgcn_hip.h"

extern "C" int ctgcn_set_error_(int code, const char *msg);   // defined in ctgcn_hip.hip

#define CTGCN_TRY(expr)                                                              \
    do {                                                                             \
        hipError_t e_ = (expr);                                                      \
        if (e_ != hipSuccess) {                                                      \
            char buf[384];                                                           \
            snprintf(buf, sizeof(buf), "%s -> %s", #expr, hipGetErrorString(e_));   \
            return ctgcn_set_error_(CTGCN_E_HIP, buf);                               \
        }                                                                            \
    } while (0)

static inline int ctgcn_fail(int code, const char *what, const char *text)
{
    char buf[224];
    snprintf(buf, sizeof(buf), "%s: %s", what, text);
    return ctgcn_set_error_(code, buf);
}

static inline bool ctgcn_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// rows of E as float4: d and the leading dimension a multiple of 4, the base 16-byte aligned
static inline int ctgcn_can_vec4(int32_t d, const float *E, int64_t lde) { return d % 4 == 0 && lde % 4 == 0 && ctgcn_aligned16(E); }

// A kernel that takes `bytes` of dynamic LDS has to opt in above 64 KiB; the CU has 160 KiB.
static inline int ctgcn_opt_in_lds(const void *fn, size_t bytes, const char *what)
{
    if (bytes > 160 * 1024) {
        char buf[96];
        snprintf(buf, sizeof(buf), "%s: LDS need above 160 KiB", what);
        return ctgcn_set_error_(CTGCN_E_UNSUPPORTED, buf);
    }
    if (bytes > 64 * 1024) CTGCN_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return CTGCN_OK;
}
