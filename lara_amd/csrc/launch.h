// launch.h -- the one checked path for kernel launches and HIP API calls of the host code.
//
// Every failure that leaves an entry point as LARA2DGS_E_LAUNCH goes through l2d_fail, which records the hipError_t that
// lara2dgs_last_hip_error() then reports (0 = hipSuccess for a failure inside the library that has no HIP error).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/lara2dgs.h"

void l2d_set_hip_error(hipError_t e);
static inline int l2d_fail(hipError_t e) {
    l2d_set_hip_error(e);
    return LARA2DGS_E_LAUNCH;
}

// optional event bracketing of a launch (see lara2dgs_profile_enable)
struct L2dProfScope {
    int slot;
    hipStream_t s;
    L2dProfScope(const char *name, hipStream_t stream);
    ~L2dProfScope();
};
#define L2D_PROF(name, stream) L2dProfScope prof_scope__(name, stream)

// a HIP API call, or a launcher of ours that returns hipError_t (launch_gemm_ring, launch_mlp_fused)
// (variadic: a call such as launch_gemm_ring<1, 4>(p, s) carries commas of its own)
#define L2D_HIP(...)                                        \
    do {                                                    \
        const hipError_t e__ = (__VA_ARGS__);               \
        if (e__ != hipSuccess) return l2d_fail(e__);        \
    } while (0)
// a failure of the library's own that no HIP call reported
#define L2D_FAIL_INTERNAL() return l2d_fail(hipSuccess)
// a call into another entry point / launcher that returns a LARA2DGS status (it has recorded its own error)
#define L2D_TRY(...)                                        \
    do {                                                    \
        const int rc__ = (__VA_ARGS__);                     \
        if (rc__ != LARA2DGS_OK) return rc__;               \
    } while (0)

// the launch as an expression of type hipError_t (for the launchers that hand the error to their caller)
#define L2D_LAUNCH_ERR(stream, kernel, grid, block, lds, ...)                  \
    ({                                                                         \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);     \
        hipGetLastError();                                                     \
    })
// checked launch inside a profile scope the caller has opened (one label over several launches), or without a label
#define L2D_LAUNCH_IN_SCOPE(stream, kernel, grid, block, lds, ...) L2D_HIP(L2D_LAUNCH_ERR(stream, kernel, grid, block, lds, __VA_ARGS__))
// checked launch under its own profile label: the scope closes before the error is read
#define L2D_LAUNCH(label, stream, kernel, grid, block, lds, ...)               \
    do {                                                                       \
        {                                                                      \
            L2D_PROF(label, stream);                                           \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__); \
        }                                                                      \
        L2D_HIP(hipGetLastError());                                            \
    } while (0)
