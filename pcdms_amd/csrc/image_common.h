// What more than one of misc.hip / image_metrics.hip / image_prep.hip / eval_nets.hip / pose_draw.hip / pose_net.hip / detect.hip / resize_cv.hip uses, and nothing else.  Internal linkage: each unit gets its own.
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

// int(v) of the reference (truncation toward zero), clamped to +-2^20 (a keypoint, a coordinate may be any float); NaN goes to the lower bound
constexpr int kCvCoord = 1 << 20;
__device__ __forceinline__ int cv_trunc(float v) {
    if (!(v > -(float)kCvCoord)) return -kCvCoord;
    if (v > (float)kCvCoord) return kCvCoord;
    return (int)v;
}

// OpenCV's 8-bit INTER_LINEAR, one axis (include/pcdm.h: pcdm_resize_linear_u8): source index and the two 11-bit weights of output d.  x axis
// (clamp_frac): the fraction is zeroed where the index is clamped; y axis: the two rows are clamped and the fraction kept.  The index goes
// through cv_trunc.
__device__ __forceinline__ void cv_lin_coeff(int d, double scale, int n_in, bool clamp_frac, int& s0, int& s1, int& w0, int& w1) {
#pragma clang fp contract(off)
    double fd = ((double)d + 0.5) * scale;
    PCDM_CV_OPAQUE(fd);
    float f = (float)(fd - 0.5);
    const float fl = floorf(f);
    int s = cv_trunc(fl);
    f = f - fl;
    if (clamp_frac) {
        if (s < 0) { f = 0.0f; s = 0; }
        if (s >= n_in - 1) { f = 0.0f; s = n_in - 1; }
    }
    w0 = (int)rintf((1.0f - f) * 2048.0f);
    w1 = (int)rintf(f * 2048.0f);
    s0 = imin(imax(s, 0), n_in - 1);
    s1 = imin(imax(s + 1, 0), n_in - 1);
}

// a window w = (x0, y0, W, H) that lies inside an Hi x Wi image: the refusal shared by every entry that takes one (include/pcdm.h)
inline bool met_window_ok(int Hi, int Wi, const int32_t* w) {
    return w && Hi > 0 && Wi > 0 && w[0] >= 0 && w[1] >= 0 && w[2] > 0 && w[3] > 0 && (int64_t)w[0] + w[2] <= Wi && (int64_t)w[1] + w[3] <= Hi;
}

inline dim3 grid1d(int64_t n, int bs) { return dim3((unsigned)((n + bs - 1) / bs)); }
}  // namespace
