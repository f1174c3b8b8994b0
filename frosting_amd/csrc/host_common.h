// What every C entry point of the library needs (api.hip: the rasterizer; api_ops.hip: everything else): the error
// record behind frg_last_error and the two early-return macros.  Internal -- not part of the installed interface.
#pragma once
#include "../../include/frosting_rasterizer.h"
#include "kernels.h"

namespace frg {

// Stores the formatted message in the calling thread's error buffer (defined in api.hip, read by frg_last_error)
// -> code, so that a failing entry point can `return fail(FRG_EINVAL, "...")`.
int fail(int code, const char* fmt, ...);

// What api.hip remembers of the forwards (its notes), for the exchange entry points of api_ops.hip: was the forward that last
// filled this geometry buffer / whose backward's phase 1 last ran on this workspace given sh_rotations?  Those entry points run
// the per-Gaussian chain without the matrices and refuse such buffers (kRotatedSingleView).
bool forward_was_rotated(const void* geom_buffer);
bool phase1_was_rotated(const void* workspace);
constexpr const char* kRotatedSingleView = "the forward that filled these buffers was given sh_rotations: rotated SH directions are a "
                                           "single-view render feature, the view-parallel exchanges do not carry them";

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
