#include "pcdm_device.h"
#include "../../include/pcdm.h"
#include "image_common.h"

// ---- input preparation of the evaluation drivers (stage2_batchtest_inpaint_model.py:135-149: Image.resize(..., BICUBIC), canvas pasting,
// ToTensor + Normalize, CLIPImageProcessor) ------------------------------------------------------------------------------------------------
// Pillow's 8-bit resampler restated: per axis a table {lo[o], count[o], int32 coeff[o][k]} of 22-bit fixed-point weights (built on the host as
// Pillow builds them, include/pcdm.h), per output byte clip8((2^21 + sum coeff * pixel) >> 22) in 32-bit integers, the horizontal pass rounded to
// uint8 before the vertical pass reads it.  The kernels know nothing about the filter.  A table comes from the caller's device memory, so every
// entry is clamped into the image before it is used: a wrong table gives wrong pixels, never an access outside src, the LDS tile or the window.
namespace {
constexpr int kRsTW = 32, kRsTH = 16;           // output tile of resample_tile_kernel
constexpr int kRsLdsBytes = 24 * 1024;          // most LDS one tile may ask for: 256 rows of 3 channels (6 workgroups a CU); beyond it: two launches
constexpr int kRsBits = 22;                     // Pillow's PRECISION_BITS for 8-bit images

struct RsAxis {            // tab == nullptr: the axis keeps its size and is copied (Pillow skips that pass)
    const int32_t* tab;    // [lo (n_out) | count (n_out) | coeff (n_out * k)]
    int n_out, k, n_in;
};
struct U8Norm { float mean[4], sd[4]; };   // u8_to_nchw_kernel's per-channel constants
__device__ __forceinline__ void rs_entry(const RsAxis& a, int o, int& lo, int& cnt) {
    if (!a.tab) { lo = o; cnt = 1; return; }
    lo = imin(imax(a.tab[o], 0), a.n_in - 1);
    cnt = imin(imax(a.tab[a.n_out + o], 0), imin(a.k, a.n_in - lo));
}
__device__ __forceinline__ const int32_t* rs_coeff(const RsAxis& a, int o) { return a.tab + 2 * (int64_t)a.n_out + (int64_t)o * a.k; }
__device__ __forceinline__ int rs_clip8(int acc) { return imin(imax(acc >> kRsBits, 0), 255); }
__host__ __device__ inline int rs_lds_pitch(int C) { return (kRsTW * C + 3) & ~3; }

// One workgroup per 32 x 16 output tile: the input rows [r0, r0 + nrows) its 16 output rows read are resampled horizontally into LDS as uint8
// (nrows x 32 C bytes: 4.1 KB for 1101 -> 512 rows, never above kRsLdsBytes: the launcher takes the two-launch form instead), then the vertical
// pass runs out of LDS four bytes per lane and writes dwords where the destination address allows.  dst is the window's first byte.
__global__ __launch_bounds__(256) void resample_tile_kernel(const uint8_t* __restrict__ src, int C, RsAxis ax, RsAxis ay, uint8_t* __restrict__ dst,
                                                            int64_t dst_pitch, int max_rows) {
    PCDM_DYN_SMEM(smem);
    uint8_t* tile = (uint8_t*)smem;
    const int tid = threadIdx.x, pitch = rs_lds_pitch(C);
    const int tx0 = blockIdx.x * kRsTW, ty0 = blockIdx.y * kRsTH;
    const int tw = imin(kRsTW, ax.n_out - tx0), th = imin(kRsTH, ay.n_out - ty0), rowb = tw * C;
    int r0, c0, rl, cl;
    rs_entry(ay, ty0, r0, c0);
    rs_entry(ay, ty0 + th - 1, rl, cl);
    const int nrows = imin(imax(r0 + c0, rl + cl) - r0, max_rows);
    for (int i = tid; i < nrows * rowb; i += 256) {               // horizontal pass: (row, column, channel), the byte index fastest
        const int row = i / rowb, e = i - row * rowb;
        const int col = e / C, c = e - col * C;
        int lo, cnt;
        rs_entry(ax, tx0 + col, lo, cnt);
        const uint8_t* p = src + ((int64_t)(r0 + row) * ax.n_in + lo) * C + c;
        int v = p[0];
        if (ax.tab) {
            const int32_t* w = rs_coeff(ax, tx0 + col);
            int acc = 1 << (kRsBits - 1);
            for (int k = 0; k < cnt; ++k) acc += w[k] * (int)p[k * C];
            v = rs_clip8(acc);
        }
        tile[row * pitch + e] = (uint8_t)v;
    }
    __syncthreads();
    const int groups = pitch / 4;
    for (int g = tid; g < th * groups; g += 256) {                // vertical pass: four bytes of one output row per lane
        const int row = g / groups, e0 = (g - row * groups) * 4;
        if (e0 >= rowb) continue;
        int lo, cnt;
        rs_entry(ay, ty0 + row, lo, cnt);
        uint32_t out;
        if (!ay.tab) {
            out = *(const uint32_t*)(tile + (lo - r0) * pitch + e0);
        } else {
            const int32_t* w = rs_coeff(ay, ty0 + row);
            int a0 = 1 << (kRsBits - 1), a1 = a0, a2 = a0, a3 = a0;
            for (int k = 0; k < cnt; ++k) {
                const int rr = lo + k - r0;
                if (rr < 0 || rr >= nrows) continue;              // (only a table that is not Pillow's)
                const uint32_t px = *(const uint32_t*)(tile + rr * pitch + e0);
                const int wk = w[k];
                a0 += wk * (int)(px & 255u);
                a1 += wk * (int)((px >> 8) & 255u);
                a2 += wk * (int)((px >> 16) & 255u);
                a3 += wk * (int)(px >> 24);
            }
            out = (uint32_t)rs_clip8(a0) | ((uint32_t)rs_clip8(a1) << 8) | ((uint32_t)rs_clip8(a2) << 16) | ((uint32_t)rs_clip8(a3) << 24);
        }
        uint8_t* d = dst + (int64_t)(ty0 + row) * dst_pitch + (int64_t)tx0 * C + e0;
        if (e0 + 4 <= rowb && ((uintptr_t)d & 3) == 0) {
            *(uint32_t*)d = out;
        } else {
            for (int j = 0; j < 4 && e0 + j < rowb; ++j) d[j] = (uint8_t)(out >> (8 * j));
        }
    }
}

// One pass of the two-launch form, one output byte per lane straight from global memory: vertical = 0: src [rows, a.n_in, C] -> dst rows of
// a.n_out pixels; vertical = 1: src [a.n_in, row_px, C] -> a.n_out rows of row_px pixels.
__global__ __launch_bounds__(256) void resample_axis_kernel(const uint8_t* __restrict__ src, int C, RsAxis a, int vertical, int rows, int row_px,
                                                            uint8_t* __restrict__ dst, int64_t dst_pitch) {
    const int rowb = row_px * C;                                  // bytes of an OUTPUT row
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * rowb) return;
    const int y = (int)(i / rowb), e = (int)(i - (int64_t)y * rowb);
    const int o = vertical ? y : e / C;
    int lo, cnt;
    rs_entry(a, o, lo, cnt);
    const int64_t step = vertical ? rowb : C;
    const uint8_t* p = vertical ? src + (int64_t)lo * rowb + e : src + ((int64_t)y * a.n_in + lo) * C + (e - o * C);
    const int32_t* w = rs_coeff(a, o);
    int acc = 1 << (kRsBits - 1);
    for (int k = 0; k < cnt; ++k) acc += w[k] * (int)p[k * step];
    dst[(int64_t)y * dst_pitch + e] = (uint8_t)rs_clip8(acc);
}

// out fp32 NCHW [1, C, H, W] <- (x - mean[c]) / std[c] of a window of a uint8 HWC image, x = float(p) / float(scale) (mode 0: ToTensor) or
// float(double(p) * scale) (mode 1: the numpy rescale of transformers' image processors); one output element per lane, stores coalesced
__global__ __launch_bounds__(256) void u8_to_nchw_kernel(const uint8_t* __restrict__ src, int Ws, int C, int x0, int y0, int W, int H, int mode,
                                                         double scale, U8Norm nm, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // over (c, y, x)
    if (i >= C * H * W) return;
    const int c = i / (H * W), r = i - c * H * W;
    const int y = r / W, x = r - y * W;
    const uint8_t p = src[((int64_t)(y0 + y) * Ws + x0 + x) * C + c];
    const float v = mode ? (float)((double)p * scale) : (float)p / (float)scale;
    out[i] = (v - nm.mean[c]) / nm.sd[c];
}

inline bool rs_axis_ok(const int32_t* tab, int k, int n_in, int n_out) { return tab ? k > 0 && k <= 1 << 20 : n_in == n_out; }
// rows of LDS the largest tile can need: lo moves by at most floor(15 n_in / n_out) + 1 over a tile's 16 outputs, the last one reads k rows
inline int64_t rs_tile_rows(int ky, int Hs, int Hd) {
    if (Hs == Hd) return kRsTH;
    const int64_t span = (int64_t)((double)(kRsTH - 1) * (double)Hs / (double)Hd) + 2 + ky;
    return span < Hs ? span : Hs;
}
}  // namespace

extern "C" int64_t pcdm_resample_ws_bytes(int Hs, int Ws, int Hd, int Wd, int channels, int ky) {
    if (Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0 || (channels != 1 && channels != 3) || (Hs != Hd && ky <= 0)) return -1;
    if (rs_tile_rows(ky, Hs, Hd) * rs_lds_pitch(channels) <= kRsLdsBytes) return 0;   // one launch
    return Ws == Wd ? 0 : (int64_t)Hs * Wd * channels;      // the horizontally resampled image between the two launches
}

extern "C" int pcdm_resample_u8(const void* src, int Hs, int Ws, int channels, const int32_t* xtab, int kx, const int32_t* ytab, int ky, void* dst,
                                int Hd, int Wd, int64_t dst_pitch, int x0, int y0, void* ws, int64_t ws_bytes, pcdm_stream_t s) {
    if (!src || !dst || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0 || (channels != 1 && channels != 3) || x0 < 0 || y0 < 0) return -1;
    if ((xtab == nullptr) != (Ws == Wd) || (ytab == nullptr) != (Hs == Hd) || !rs_axis_ok(xtab, kx, Ws, Wd) || !rs_axis_ok(ytab, ky, Hs, Hd)) return -1;
    if (dst_pitch < ((int64_t)x0 + Wd) * channels || (int64_t)Hs * Ws * channels >= (int64_t)1 << 31 || (int64_t)Hd * Wd * channels >= (int64_t)1 << 31) return -1;
    const int C = channels;
    const RsAxis ax{xtab, Wd, kx, Ws}, ay{ytab, Hd, ky, Hs};
    uint8_t* win = (uint8_t*)dst + (int64_t)y0 * dst_pitch + (int64_t)x0 * C;
    const int64_t rows = rs_tile_rows(ky, Hs, Hd);
    if (rows * rs_lds_pitch(C) <= kRsLdsBytes) {
        PCDM_LAUNCH(resample_tile_kernel, dim3((Wd + kRsTW - 1) / kRsTW, (Hd + kRsTH - 1) / kRsTH), dim3(256), (int)rows * rs_lds_pitch(C), (hipStream_t)s,
                    (const uint8_t*)src, C, ax, ay, win, dst_pitch, (int)rows);
        PCDM_CHECK_LAUNCH();
        return 0;
    }
    const uint8_t* mid = (const uint8_t*)src;               // rows too far apart for a tile: horizontal pass to the workspace, then the vertical pass
    if (xtab) {
        if (!ws || ws_bytes < (int64_t)Hs * Wd * C) return -1;
        PCDM_LAUNCH(resample_axis_kernel, grid1d((int64_t)Hs * Wd * C, 256), dim3(256), 0, (hipStream_t)s, (const uint8_t*)src, C, ax, 0, Hs, Wd, (uint8_t*)ws,
                    (int64_t)Wd * C);
        PCDM_CHECK_LAUNCH();
        mid = (const uint8_t*)ws;
    }
    PCDM_LAUNCH(resample_axis_kernel, grid1d((int64_t)Hd * Wd * C, 256), dim3(256), 0, (hipStream_t)s, mid, C, ay, 1, Hd, Wd, win, dst_pitch);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_u8_to_nchw(const void* src_u8, int Hs, int Ws, int channels, const int32_t* win, int mode, double scale, const float* mean,
                               const float* std_, float* out, pcdm_stream_t s) {
    if (!src_u8 || !out || (channels != 1 && channels != 3) || !met_window_ok(Hs, Ws, win) || !mean || !std_ || (mode != 0 && mode != 1)) return -1;
    if (!(scale > 0.0) || (int64_t)win[2] * win[3] * channels >= (int64_t)1 << 31 || (int64_t)Hs * Ws * channels >= (int64_t)1 << 31) return -1;
    U8Norm nm{};
    for (int c = 0; c < channels; ++c) {
        nm.mean[c] = mean[c];
        nm.sd[c] = std_[c];
    }
    PCDM_LAUNCH(u8_to_nchw_kernel, grid1d((int64_t)win[2] * win[3] * channels, 256), dim3(256), 0, (hipStream_t)s, (const uint8_t*)src_u8, Ws, channels,
                win[0], win[1], win[2], win[3], mode, scale, nm, out);
    PCDM_CHECK_LAUNCH();
    return 0;
}

// ---- the OpenCV-cubic resize of the reference's metric scripts (metrics.py: calculate_from_disk resizes both images before it scores them; the
// scores: image_metrics.hip) ---------------------------------------------------------------------------------------------------------------------
// cv2.resize(float32 image, INTER_CUBIC) restated (resizeGeneric_ with HResizeCubic / VResizeCubic, float work type): per axis scale =
// 1 / (n_out / n_in) in double, f = float((d + 0.5) scale - 0.5), s = floor(f), t = f - s in fp32, taps s - 1 .. s + 2 clamped into the image, the
// Keys coefficients with A = -0.75 in fp32, the horizontal pass first.  No antialiasing, no rounding, no clipping.  Every fp32 / fp64 operation
// below is a separate IEEE operation (cv_mul): a fused multiply-add would round once where OpenCV's C++ rounds twice.
namespace {
constexpr int kCvTW = 32, kCvTH = 16;           // output tile of resize_cubic_kernel
constexpr int kCvRows = 4 * kCvTH;              // LDS rows of a tile: a contiguous span of source rows, or four rows per output row

__device__ __forceinline__ void cv_cubic_coeffs(int d, double scale, int& s, float c[4]) {
#pragma clang fp contract(off)
    double fd = ((double)d + 0.5) * scale;
    PCDM_CV_OPAQUE(fd);
    const float f = (float)(fd - 0.5);
    const float fl = floorf(f);
    const float t = f - fl;
    s = (int)fl;
    const float A = -0.75f;
    const float t1 = t + 1.0f, t2 = 1.0f - t;
    c[0] = cv_mul(cv_mul(cv_mul(A, t1) - 5.0f * A, t1) + 8.0f * A, t1) - 4.0f * A;
    c[1] = cv_mul(cv_mul(cv_mul(A + 2.0f, t) - (A + 3.0f), t), t) + 1.0f;
    c[2] = cv_mul(cv_mul(cv_mul(A + 2.0f, t2) - (A + 3.0f), t2), t2) + 1.0f;
    c[3] = 1.0f - c[0] - c[1] - c[2];
}
__device__ __forceinline__ float cv_tap4(float a, float b, float c, float d, const float* w) {
#pragma clang fp contract(off)
    return cv_mul(a, w[0]) + cv_mul(b, w[1]) + cv_mul(c, w[2]) + cv_mul(d, w[3]);
}
__device__ __forceinline__ float cv_load(const void* src, int f32, int64_t i) { return f32 ? ((const float*)src)[i] : (float)((const uint8_t*)src)[i]; }

// One workgroup per 32 x 16 output tile of image `index`.  The tile's coefficient tables go to LDS first; then the horizontally filtered source
// rows (fp32, 32 pixels x 3 channels each): the contiguous span [s(first) - 1, s(last) + 2] when it has at most 64 rows (every enlargement, and
// reductions up to about 4 : 1), else the four tap rows of each output row (64 rows: without antialiasing an output row never reads more); then the
// vertical pass out of LDS.  Source rows and columns are clamped into the image (edge replication), LDS rows into the staged rows.
__global__ __launch_bounds__(256) void resize_cubic_kernel(const void* __restrict__ src, int f32, int Hs, int Ws, double scale_x, double scale_y,
                                                           float* __restrict__ dst, int Hd, int Wd, int nchw, float divisor) {
    __shared__ float tile[kCvRows * kCvTW * 3];
    __shared__ float cx[kCvTW][4], cy[kCvTH][4];
    __shared__ int sx[kCvTW], sy[kCvTH];
    const int tid = threadIdx.x;
    const int tx0 = blockIdx.x * kCvTW, ty0 = blockIdx.y * kCvTH;
    const int tw = imin(kCvTW, Wd - tx0), th = imin(kCvTH, Hd - ty0);
    if (tid < kCvTW) {
        cv_cubic_coeffs(imin(tx0 + tid, Wd - 1), scale_x, sx[tid], cx[tid]);
    } else if (tid >= 64 && tid < 64 + kCvTH) {
        cv_cubic_coeffs(imin(ty0 + tid - 64, Hd - 1), scale_y, sy[tid - 64], cy[tid - 64]);
    }
    __syncthreads();
    const int base = sy[0] - 1;
    const int span = sy[th - 1] + 2 - base + 1;
    const bool contiguous = span >= 4 && span <= kCvRows;
    const int nrows = contiguous ? span : 4 * th;
    const int rowe = tw * 3;
    for (int i = tid; i < nrows * rowe; i += 256) {               // horizontal pass: (row, column, channel), the channel fastest
        const int row = i / rowe, e = i - row * rowe;
        const int col = e / 3, c = e - col * 3;
        const int r = contiguous ? base + row : sy[row >> 2] - 1 + (row & 3);
        const int64_t p = (int64_t)imin(imax(r, 0), Hs - 1) * Ws;
        const int s = sx[col];
        const float a0 = cv_load(src, f32, (p + imin(imax(s - 1, 0), Ws - 1)) * 3 + c);
        const float a1 = cv_load(src, f32, (p + imin(imax(s, 0), Ws - 1)) * 3 + c);
        const float a2 = cv_load(src, f32, (p + imin(imax(s + 1, 0), Ws - 1)) * 3 + c);
        const float a3 = cv_load(src, f32, (p + imin(imax(s + 2, 0), Ws - 1)) * 3 + c);
        tile[row * (kCvTW * 3) + e] = cv_tap4(a0, a1, a2, a3, cx[col]);
    }
    __syncthreads();
    for (int i = tid; i < th * rowe; i += 256) {                  // vertical pass; the store index fastest in the destination's layout
        int row, col, c;
        if (nchw) {
            c = i / (th * tw);
            const int r2 = i - c * th * tw;
            row = r2 / tw;
            col = r2 - row * tw;
        } else {
            row = i / rowe;
            const int e = i - row * rowe;
            col = e / 3;
            c = e - col * 3;
        }
        const int l0 = contiguous ? sy[row] - 1 - base : 4 * row;
        const int e = col * 3 + c;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = tile[imin(imax(l0 + k, 0), nrows - 1) * (kCvTW * 3) + e];
        float o = cv_tap4(v[0], v[1], v[2], v[3], cy[row]);
        if (divisor > 0.f) o = o / divisor;
        const int y = ty0 + row, x = tx0 + col;
        dst[nchw ? ((int64_t)c * Hd + y) * Wd + x : ((int64_t)y * Wd + x) * 3 + c] = o;
    }
}
}  // namespace

extern "C" int pcdm_resize_cubic_f32(const void* src, int src_is_f32, int Hs, int Ws, int channels, float* dst, int N, int Hd, int Wd, int index,
                                     int nchw, float divisor, pcdm_stream_t s) {
    if (!src || !dst || channels != 3 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0 || N <= 0 || index < 0 || index >= N) return -1;
    if (((uintptr_t)dst & 3) || (src_is_f32 && ((uintptr_t)src & 3))) return -1;
    if ((int64_t)Hs * Ws * 3 >= (int64_t)1 << 31 || (int64_t)Hd * Wd * 3 >= (int64_t)1 << 31 || (Hd + kCvTH - 1) / kCvTH > 65535) return -1;
    const double scale_x = 1.0 / ((double)Wd / (double)Ws), scale_y = 1.0 / ((double)Hd / (double)Hs);
    PCDM_LAUNCH(resize_cubic_kernel, dim3((Wd + kCvTW - 1) / kCvTW, (Hd + kCvTH - 1) / kCvTH), dim3(256), 0, (hipStream_t)s, src, src_is_f32 != 0, Hs, Ws,
                scale_x, scale_y, dst + (int64_t)index * Hd * Wd * 3, Hd, Wd, nchw != 0, divisor);
    PCDM_CHECK_LAUNCH();
    return 0;
}
