// What more than one of misc.hip / image_metrics.hip / image_prep.hip / eval_nets.hip / pose_draw.hip uses, and nothing else.  Internal linkage: each unit gets its own.
#pragma once
#include "pcdm_device.h"

namespace {
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// a * b as an IEEE product of its own: under -ffp-contract=fast the backend fuses any multiply into the add that consumes it (a pragma does not
// stop it), so the product passes through an empty asm statement, which the add cannot see through
#ifdef PCDM_EMU
#define PCDM_CV_OPAQUE(x) ((void)0)
#else
#define PCDM_CV_OPAQUE(x) asm volatile("" : "+v"(x))
#endif
__device__ __forceinline__ float cv_mul(float a, float b) {
#pragma clang fp contract(off)
    float p = a * b;
    PCDM_CV_OPAQUE(p);
    return p;
}

// a window w = (x0, y0, W, H) that lies inside an Hi x Wi image: the refusal shared by every entry that takes one (include/pcdm.h)
inline bool met_window_ok(int Hi, int Wi, const int32_t* w) {
    return w && Hi > 0 && Wi > 0 && w[0] >= 0 && w[1] >= 0 && w[2] > 0 && w[3] > 0 && (int64_t)w[0] + w[2] <= Wi && (int64_t)w[1] + w[3] <= Hi;
}

inline dim3 grid1d(int64_t n, int bs) { return dim3((unsigned)((n + bs - 1) / bs)); }
}  // namespace
