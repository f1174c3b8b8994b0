// What every C entry point of the library needs (api.hip: the rasterizer; api_ops.hip: everything else): the error
// record behind frg_last_error and the two early-return macros.  Internal -- not part of the installed interface.
#pragma once
#include "../../include/frosting_rasterizer.h"
#include "kernels.h"

namespace frg {

// Stores the formatted message in the calling thread's error buffer (defined in api.hip, read by frg_last_error)
// -> code, so that a failing entry point can `return fail(FRG_EINVAL, "...")`.
int fail(int code, const char* fmt, ...);

// spin-wait hint of the mailbox polls (the host side is not tied to x86)
inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__) || defined(__arm__)
    __asm__ __volatile__("yield");
#else
    __asm__ __volatile__("" ::: "memory");
#endif
}

}  // namespace frg

// a negative return code leaves the function
#define FRG_TRY(expr)                  \
    do {                               \
        const int rc_ = (expr);        \
        if (rc_ < 0) return rc_;       \
    } while (0)

#define FRG_HIP(call)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) return frg::fail(FRG_EHIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)
