#include "pcdm_device.h"
#include "../../include/pcdm.h"
#include "image_common.h"
#include <float.h>

// ---- cv2.resize(uint8 image, INTER_LANCZOS4 | INTER_AREA) restated: the frame controlnet_aux's resize_image gives both pose networks -------------
// Four arithmetic forms (include/pcdm.h: pcdm_resize_cv_u8): Lanczos4 and the two-tap bilinear that INTER_AREA becomes when an axis enlarges share
// one tap kernel (8 or 2 integer coefficients per output and axis, from the caller's tables); INTER_AREA on integer ratios is a box sum without
// tables; true INTER_AREA reads (source, fp32 weight) lists.  One output pixel per lane, every lane recomputes its own taps: the work is a
// megapixel and launch-bound.  A table comes from the caller's device memory, so every entry is clamped before it is used: a wrong table gives
// wrong pixels, never an access outside src or dst.  The fp32 form keeps every multiply and add its own IEEE operation (cv_mul).
namespace {
enum { kCvLanczos4 = 0, kCvAreaInt = 1, kCvArea = 2, kCvAreaLinear = 3 };

__device__ __forceinline__ uint8_t cv_sat8(float v) {           // saturate_cast<uchar>(float): rint (ties to even), then saturation; NaN -> 0
    return (uint8_t)(int)fminf(fmaxf(rintf(v), 0.0f), 255.0f);
}
__device__ __forceinline__ void cv_pixel(int64_t i, int Hd, int Wd, int& x, int& y, int& m) {
    x = (int)(i % Wd);
    y = (int)((i / Wd) % Hd);
    m = (int)(i / ((int64_t)Wd * Hd));
}

// Rules (a) and (d).  Table of an axis: [s (n_out) | coeff (n_out * TAPS)]; tap k reads source s - (TAPS / 2 - 1) + k, clamped into the image.
// TAPS 8: S = sum src alpha in int32, out = clip8((sum S beta + 2^21) >> 22), the vertical sum in 64 bits; coefficients saturate to int16.
// TAPS 2: pcdm_resize_linear_u8's form; coefficients are clamped into [0, 2048], so no intermediate leaves int32.
template <int TAPS>
__global__ __launch_bounds__(256) void resize_cv_taps_kernel(const uint8_t* __restrict__ src, int M, int Hs, int Ws, const int32_t* __restrict__ xtab,
                                                             const int32_t* __restrict__ ytab, uint8_t* __restrict__ dst, int Hd, int Wd) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)M * Hd * Wd) return;
    int x, y, m;
    cv_pixel(i, Hd, Wd, x, y, m);
    constexpr int kLo = TAPS == 8 ? -32768 : 0, kHi = TAPS == 8 ? 32767 : 2048, kBack = TAPS / 2 - 1;
    const int sx = imin(imax(xtab[x], -TAPS), Ws + TAPS), sy = imin(imax(ytab[y], -TAPS), Hs + TAPS);
    const int32_t* ca = xtab + Wd + (int64_t)x * TAPS;
    const int32_t* cb = ytab + Hd + (int64_t)y * TAPS;
    int xi[TAPS], a[TAPS];
#pragma unroll
    for (int k = 0; k < TAPS; ++k) {
        xi[k] = imin(imax(sx - kBack + k, 0), Ws - 1) * 3;
        a[k] = imin(imax(ca[k], kLo), kHi);
    }
    const uint8_t* img = src + (int64_t)m * Hs * Ws * 3;
    if constexpr (TAPS == 8) {
        int64_t acc[3] = {0, 0, 0};
        for (int j = 0; j < TAPS; ++j) {
            const uint8_t* row = img + (int64_t)imin(imax(sy - kBack + j, 0), Hs - 1) * Ws * 3;
            const int b = imin(imax(cb[j], kLo), kHi);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                int S = 0;
#pragma unroll
                for (int k = 0; k < TAPS; ++k) S += (int)row[xi[k] + c] * a[k];
                acc[c] += (int64_t)S * b;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t v = (acc[c] + ((int64_t)1 << 21)) >> 22;
            dst[i * 3 + c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
    } else {
        const uint8_t* r0 = img + (int64_t)imin(imax(sy, 0), Hs - 1) * Ws * 3;
        const uint8_t* r1 = img + (int64_t)imin(imax(sy + 1, 0), Hs - 1) * Ws * 3;
        const int b0 = imin(imax(cb[0], kLo), kHi), b1 = imin(imax(cb[1], kLo), kHi);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int S0 = (int)r0[xi[0] + c] * a[0] + (int)r0[xi[1] + c] * a[1];
            const int S1 = (int)r1[xi[0] + c] * a[0] + (int)r1[xi[1] + c] * a[1];
            const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
            dst[i * 3 + c] = (uint8_t)imin(imax(v, 0), 255);
        }
    }
}

// Rule (b): the sx x sy box of every output (Ws = sx Wd, Hs = sy Hd: the launcher checked); 2 x 2 in integers, any other box through one fp32 multiply.
__global__ __launch_bounds__(256) void resize_cv_area_int_kernel(const uint8_t* __restrict__ src, int M, int Hs, int Ws, int sx, int sy, float inv,
                                                                 uint8_t* __restrict__ dst, int Hd, int Wd) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)M * Hd * Wd) return;
    int x, y, m;
    cv_pixel(i, Hd, Wd, x, y, m);
    const uint8_t* p = src + (((int64_t)m * Hs + (int64_t)y * sy) * Ws + (int64_t)x * sx) * 3;
    int sum[3] = {0, 0, 0};
    for (int j = 0; j < sy; ++j, p += (int64_t)Ws * 3)
        for (int k = 0; k < sx * 3; k += 3) {
            sum[0] += p[k];
            sum[1] += p[k + 1];
            sum[2] += p[k + 2];
        }
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[i * 3 + c] = (sx == 2 && sy == 2) ? (uint8_t)((sum[c] + 2) >> 2) : cv_sat8(cv_mul((float)sum[c], inv));
}

// Rule (c).  Table of an axis: [count (n_out) | source (n_out * k) | weight, fp32 bits (n_out * k)]; count is clamped into [0, k], a source into
// the image.  Per source row of the output row, in table order: buf = 0, buf = buf + src alpha entry by entry; sum = beta buf, then sum + beta buf.
__global__ __launch_bounds__(256) void resize_cv_area_kernel(const uint8_t* __restrict__ src, int M, int Hs, int Ws, const int32_t* __restrict__ xtab, int kx,
                                                             const int32_t* __restrict__ ytab, int ky, uint8_t* __restrict__ dst, int Hd, int Wd) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)M * Hd * Wd) return;
    int x, y, m;
    cv_pixel(i, Hd, Wd, x, y, m);
    const int cx = imin(imax(xtab[x], 0), kx), cy = imin(imax(ytab[y], 0), ky);
    const int32_t* xs = xtab + Wd + (int64_t)x * kx;
    const int32_t* xw = xs + (int64_t)Wd * kx;
    const int32_t* ys = ytab + Hd + (int64_t)y * ky;
    const int32_t* yw = ys + (int64_t)Hd * ky;
    const uint8_t* img = src + (int64_t)m * Hs * Ws * 3;
    float sum[3] = {0.0f, 0.0f, 0.0f};
    for (int j = 0; j < cy; ++j) {
        const uint8_t* row = img + (int64_t)imin(imax(ys[j], 0), Hs - 1) * Ws * 3;
        const float beta = __builtin_bit_cast(float, yw[j]);
        float buf[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < cx; ++k) {
            const uint8_t* q = row + imin(imax(xs[k], 0), Ws - 1) * 3;
            const float alpha = __builtin_bit_cast(float, xw[k]);
#pragma unroll
            for (int c = 0; c < 3; ++c) buf[c] = buf[c] + cv_mul((float)q[c], alpha);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] = j == 0 ? cv_mul(beta, buf[c]) : sum[c] + cv_mul(beta, buf[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[i * 3 + c] = cv_sat8(sum[c]);
}

// equal sizes: cv2 returns the source; eight bytes per lane
__global__ __launch_bounds__(256) void resize_cv_copy_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int64_t n) {
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    for (int64_t i = i0; i < n && i < i0 + 8; ++i) dst[i] = src[i];
}

// scale = 1 / (n_out / n_in) is an integer >= 1 "within DBL_EPSILON" (cv2's is_area_fast) and the box tiles the source exactly
bool cv_int_ratio(int n_in, int n_out, int& ratio) {
    const double scale = 1.0 / ((double)n_out / (double)n_in);
    ratio = (int)scale;
    return ratio >= 1 && fabs(scale - (double)ratio) < DBL_EPSILON && (int64_t)ratio * n_out == n_in;
}
}  // namespace

extern "C" int pcdm_resize_cv_u8(const void* src, int M, int Hs, int Ws, void* dst, int Hd, int Wd, int rule, const int32_t* xtab, const int32_t* ytab,
                                 pcdm_stream_t s) {
    if (!src || !dst || M < 0 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0 || rule < kCvLanczos4 || rule > kCvAreaLinear) return -1;
    if ((int64_t)M * Hs * Ws * 3 >= (int64_t)1 << 31 || (int64_t)M * Hd * Wd * 3 >= (int64_t)1 << 31) return -1;
    if (M == 0) return 0;
    const uint8_t* in = (const uint8_t*)src;
    uint8_t* out = (uint8_t*)dst;
    const dim3 grid = grid1d((int64_t)M * Hd * Wd, 256);
    if (Hs == Hd && Ws == Wd) {
        const int64_t n = (int64_t)M * Hs * Ws * 3;
        PCDM_LAUNCH(resize_cv_copy_kernel, grid1d((n + 7) / 8, 256), dim3(256), 0, (hipStream_t)s, in, out, n);
    } else if (rule == kCvAreaInt) {
        int sx, sy;
        if (!cv_int_ratio(Ws, Wd, sx) || !cv_int_ratio(Hs, Hd, sy) || (int64_t)sx * sy > (int64_t)1 << 23) return -1;
        PCDM_LAUNCH(resize_cv_area_int_kernel, grid, dim3(256), 0, (hipStream_t)s, in, M, Hs, Ws, sx, sy, 1.0f / (float)(sx * sy), out, Hd, Wd);
    } else if (!xtab || !ytab) {
        return -1;
    } else if (rule == kCvArea) {
        const double scale_x = 1.0 / ((double)Wd / (double)Ws), scale_y = 1.0 / ((double)Hd / (double)Hs);
        if (!(scale_x >= 1.0) || !(scale_y >= 1.0)) return -1;
        PCDM_LAUNCH(resize_cv_area_kernel, grid, dim3(256), 0, (hipStream_t)s, in, M, Hs, Ws, xtab, (int)scale_x + 2, ytab, (int)scale_y + 2, out, Hd, Wd);
    } else if (rule == kCvLanczos4) {
        PCDM_LAUNCH(resize_cv_taps_kernel<8>, grid, dim3(256), 0, (hipStream_t)s, in, M, Hs, Ws, xtab, ytab, out, Hd, Wd);
    } else {
        PCDM_LAUNCH(resize_cv_taps_kernel<2>, grid, dim3(256), 0, (hipStream_t)s, in, M, Hs, Ws, xtab, ytab, out, Hd, Wd);
    }
    PCDM_CHECK_LAUNCH();
    return 0;
}
