#include "pcdm_device.h"
#include "../../include/pcdm.h"
#include "image_common.h"

// ---- image metrics of the evaluation drivers (stage2_batchtest_inpaint_model.py:203-219: the best-of-N pick by Gaussian-weighted SSIM) ---------
// A batch of N candidates against one reference (or one per candidate), each a WINDOW (x0, y0, W, H) into uint8 / fp32 NHWC images with 3
// channels, scored where the decoder left them.  skimage.metrics.structural_similarity(gaussian_weights=True, use_sample_covariance=False):
// separable Gaussian of radius r = int(3.5 sigma + 0.5), five filtered moments per channel, SSIM map averaged over the interior
// [r, H - r) x [r, W - r) -- so every tap of every averaged pixel lies inside the window and the filter's boundary mode never enters.
// Numerics: both images are centred by the midpoint of their own min / max (met_range_kernel) before the second moments are formed -- the
// covariances do not depend on the shift, the means get it added back -- and the moments accumulate in fp64: a constant image gives exact
// zeros (so constant against constant is 0/0 = NaN for ANY constant, as the formula says), a near-constant one loses nothing to E[x^2] - mu^2.
// No atomics: per-workgroup partials in a caller-provided workspace, added per image in a fixed order by one last launch (bit-identical reruns).
namespace {
constexpr int kMetSlices = 32;                  // row slices per image of the min / max and squared-error passes
constexpr int kSsimTW = 32, kSsimTH = 16;       // output tile of ssim_tile_kernel
constexpr int kSsimMaxR = 8;

struct MetImg {            // window into [n, Hi, Wi, 3]
    const void* p;
    int64_t img_stride;    // elements between images; 0: the same image for every candidate
    int Wi, x0, y0;
};
struct SsimTaps { double w[2 * kSsimMaxR + 1]; };

__device__ __forceinline__ float met_load(const MetImg& im, int f32, int n, int y, int x3) {
    const int64_t i = (int64_t)n * im.img_stride + ((int64_t)(im.y0 + y) * im.Wi + im.x0) * 3 + x3;
    return f32 ? ((const float*)im.p)[i] : (float)((const uint8_t*)im.p)[i];
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ws_range[(img * kMetSlices + slice) * 2] = {min, max} over the slice's rows, all channels; img < N: candidates, then the references
__global__ __launch_bounds__(256) void met_range_kernel(MetImg cand, MetImg ref, int N, int f32, int W, int H, float* __restrict__ ws_range) {
    __shared__ float red[2][4];
    const int img = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x;
    const int n = img < N ? img : img - N;
    const int rows = (H + kMetSlices - 1) / kMetSlices;
    const int ya = sl * rows, yb = imin(H, ya + rows);
    float mn = INFINITY, mx = -INFINITY;
    const MetImg im = img < N ? cand : ref;
    const int row_elems = 3 * W, total = (yb - ya) * row_elems;
    for (int e0 = tid; e0 < total; e0 += 256 * 8) {     // eight independent loads in flight per lane (an element past the end is clamped: a repeat)
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = imin(e0 + 256 * j, total - 1);
            const int y = e / row_elems;
            v[j] = met_load(im, f32, n, ya + y, e - y * row_elems);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            mn = fminf(mn, v[j]);
            mx = fmaxf(mx, v[j]);
        }
    }
    mn = -wave_max(-mn);
    mx = wave_max(mx);
    if ((tid & 63) == 0) { red[0][tid >> 6] = mn; red[1][tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0) {
        ws_range[(img * kMetSlices + sl) * 2 + 0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
        ws_range[(img * kMetSlices + sl) * 2 + 1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    }
}

// One workgroup per (candidate, 32 x 16 output tile).  LDS: the (16 + 2r) x (32 + 2r) halo tile of both images, three channels, centred fp32
// (24 (16 + 2r)(32 + 2r) bytes), and the row-filtered moments of one channel in fp64 (5 * 8 * 32 (16 + 2r) bytes): 53.8 KB at r = 4, 77.8 KB at r = 8.
__global__ __launch_bounds__(256) void ssim_tile_kernel(MetImg cand, MetImg ref, int N, int f32, int W, int H, int r, SsimTaps taps, float data_range,
                                                        const float* __restrict__ ws_range, double* __restrict__ ws_part) {
    PCDM_DYN_SMEM(smem);
    __shared__ float s_rng[4];     // candidate min, max; reference min, max
    __shared__ double s_red[4];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int TWH = kSsimTW + 2 * r, THH = kSsimTH + 2 * r;
    float* tile = (float*)smem;                                       // [2][3][THH][TWH]
    double* hb = (double*)(smem + (size_t)6 * THH * TWH * sizeof(float));   // [5][THH][kSsimTW]
    if (tid < 64) {
        const int which = tid >> 5, sl = tid & 31;
        const int img = which ? N + (ref.img_stride ? n : 0) : n;
        float mn = ws_range[(img * kMetSlices + sl) * 2], mx = ws_range[(img * kMetSlices + sl) * 2 + 1];
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, m, 64));
            mx = fmaxf(mx, __shfl_xor(mx, m, 64));
        }
        if (sl == 0) { s_rng[which * 2] = mn; s_rng[which * 2 + 1] = mx; }
    }
    __syncthreads();
    const float ca = 0.5f * (s_rng[0] + s_rng[1]), cb = 0.5f * (s_rng[2] + s_rng[3]);
    const double R = data_range >= 0.f ? (double)data_range : (double)s_rng[1] - (double)s_rng[0];
    const double c1 = (0.01 * R) * (0.01 * R), c2 = (0.03 * R) * (0.03 * R);
    const int tx0 = blockIdx.x * kSsimTW, ty0 = blockIdx.y * kSsimTH;   // window coordinates of the halo tile's corner
    const int row3 = TWH * 3;
#pragma unroll 4
    for (int i = tid; i < THH * row3; i += 256) {
        const int row = i / row3, c3 = i - row * row3;
        const int px = c3 / 3, c = c3 - px * 3;
        const int gy = imin(ty0 + row, H - 1), gx = imin(tx0 + px, W - 1);   // (clamped: only tiles cut by the window's edge, outputs masked below)
        tile[(c * THH + row) * TWH + px] = met_load(cand, f32, n, gy, gx * 3 + c) - ca;
        tile[((3 + c) * THH + row) * TWH + px] = met_load(ref, f32, n, gy, gx * 3 + c) - cb;
    }
    __syncthreads();
    double acc = 0.0;
    for (int c = 0; c < 3; ++c) {
        const float* tx = tile + c * THH * TWH;
        const float* ty = tile + (3 + c) * THH * TWH;
        for (int o = tid; o < THH * kSsimTW; o += 256) {            // rows: E[x], E[y], E[xx], E[yy], E[xy] of the centred values
            const int row = o / kSsimTW, col = o - row * kSsimTW;
            double m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0;
            for (int k = 0; k <= 2 * r; ++k) {
                const double w = taps.w[k], x = tx[row * TWH + col + k], y = ty[row * TWH + col + k];
                const double wx = w * x, wy = w * y;
                m0 += wx; m1 += wy; m2 += wx * x; m3 += wy * y; m4 += wx * y;
            }
            hb[(0 * THH + row) * kSsimTW + col] = m0;
            hb[(1 * THH + row) * kSsimTW + col] = m1;
            hb[(2 * THH + row) * kSsimTW + col] = m2;
            hb[(3 * THH + row) * kSsimTW + col] = m3;
            hb[(4 * THH + row) * kSsimTW + col] = m4;
        }
        __syncthreads();
        for (int o = tid; o < kSsimTH * kSsimTW; o += 256) {        // columns, then the SSIM map of this output pixel
            const int row = o / kSsimTW, col = o - row * kSsimTW;
            double m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0;
            for (int k = 0; k <= 2 * r; ++k) {
                const double w = taps.w[k];
                m0 += w * hb[(0 * THH + row + k) * kSsimTW + col];
                m1 += w * hb[(1 * THH + row + k) * kSsimTW + col];
                m2 += w * hb[(2 * THH + row + k) * kSsimTW + col];
                m3 += w * hb[(3 * THH + row + k) * kSsimTW + col];
                m4 += w * hb[(4 * THH + row + k) * kSsimTW + col];
            }
            if (tx0 + r + col < W - r && ty0 + r + row < H - r) {
                const double ux = m0 + (double)ca, uy = m1 + (double)cb;
                const double vx = m2 - m0 * m0, vy = m3 - m1 * m1, vxy = m4 - m0 * m1;
                acc += ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
            }
        }
        __syncthreads();
    }
    acc = wave_sum_f64(acc);
    if ((tid & 63) == 0) s_red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0)
        ws_part[((int64_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// scores[n] = (sum of the candidate's tile partials, in index order per lane, then the butterfly) / (3 * interior pixels); then np.argmax:
// the first maximum wins and a NaN ranks as the maximum
__global__ __launch_bounds__(256) void ssim_final_kernel(const double* __restrict__ ws_part, int N, int tiles, double inv_count, float* scores,
                                                         int32_t* argmax) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int n0 = 0; n0 < N; n0 += 4) {
        const int n = n0 + wave;
        double s = 0.0;
        if (n < N)
            for (int t = lane; t < tiles; t += 64) s += ws_part[(int64_t)n * tiles + t];
        s = wave_sum_f64(s);
        if (lane == 0 && n < N) scores[n] = (float)(s * inv_count);
    }
    __syncthreads();
    if (threadIdx.x == 0 && argmax) {
        int best = 0;
        float vb = scores[0];
        for (int i = 1; i < N && vb == vb; ++i) {
            const float v = scores[i];
            if (v != v || v > vb) { best = i; vb = v; }
        }
        *argmax = best;
    }
}

// ws_sq[n * kMetSlices + slice] = sum of squared differences over the slice's rows: integer accumulation for uint8 (exact: the partial is an
// integer below 2^53), fp64 for fp32 inputs
__global__ __launch_bounds__(256) void met_sqerr_kernel(MetImg cand, MetImg ref, int f32, int W, int H, double* __restrict__ ws_sq) {
    __shared__ double red[4];
    const int n = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x;
    const int rows = (H + kMetSlices - 1) / kMetSlices;
    const int ya = sl * rows, yb = imin(H, ya + rows);
    unsigned long long si = 0;
    double sd = 0.0;
    for (int y = ya; y < yb; ++y)
        for (int x3 = tid; x3 < 3 * W; x3 += 256) {
            const float a = met_load(cand, f32, n, y, x3), b = met_load(ref, f32, n, y, x3);
            if (f32) {
                const double d = (double)a - (double)b;
                sd += d * d;
            } else {
                const int d = (int)a - (int)b;
                si += (unsigned long long)(d * d);
            }
        }
    const double s = wave_sum_f64(f32 ? sd : (double)si);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) ws_sq[n * kMetSlices + sl] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void psnr_final_kernel(const double* __restrict__ ws_sq, int N, double inv_count, double R, float* __restrict__ mse_out,
                                  float* __restrict__ psnr_out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s = 0.0;
    for (int i = 0; i < kMetSlices; ++i) s += ws_sq[n * kMetSlices + i];
    const double mse = s * inv_count;
    if (mse_out) mse_out[n] = (float)mse;
    if (psnr_out) psnr_out[n] = (float)(10.0 * log10(R * R / mse));
}

// out <- the window of cand[*index_dev]: uint8 [H, W, 3], or fp32 NCHW [1, 3, H, W] = (x / 255 - 0.5) / 0.5 (ToTensor + Normalize([0.5], [0.5]))
__global__ void select_image_kernel(const uint8_t* __restrict__ cand, int N, int Hc, int Wc, int x0, int y0, int W, int H,
                                    const int32_t* __restrict__ index_dev, void* __restrict__ out, int normalized) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // over (y, x, c)
    if (i >= H * W * 3) return;
    const int n = imin(imax(*index_dev, 0), N - 1);
    const int y = i / (3 * W), r3 = i - y * 3 * W;
    const int x = r3 / 3, c = r3 - x * 3;
    const uint8_t v = cand[(((int64_t)n * Hc + y0 + y) * Wc + x0 + x) * 3 + c];
    if (!normalized) ((uint8_t*)out)[i] = v;
    else ((float*)out)[((int64_t)c * H + y) * W + x] = ((float)v / 255.0f - 0.5f) / 0.5f;
}

// the refusals shared by pcdm_ssim / pcdm_psnr / pcdm_absdiff / pcdm_ssim_box (include/pcdm.h)
inline bool met_args_ok(const void* cand, int N, int Hc, int Wc, const int32_t* cw, const void* ref, int ref_n, int Hr, int Wr, const int32_t* rw,
                        int channels) {
    if (!cand || !ref || N <= 0 || N > 65535 || (ref_n != 1 && ref_n != N) || channels != 3) return false;
    if (!met_window_ok(Hc, Wc, cw) || !met_window_ok(Hr, Wr, rw) || cw[2] != rw[2] || cw[3] != rw[3]) return false;
    return (int64_t)cw[2] * cw[3] * 3 < (int64_t)1 << 31 && (int64_t)Hc * Wc * 3 < (int64_t)1 << 31 && (int64_t)Hr * Wr * 3 < (int64_t)1 << 31;
}
inline int ssim_radius(float sigma) { return sigma > 0.f && sigma < 1e3f ? (int)(3.5f * sigma + 0.5f) : -1; }
inline MetImg met_img(const void* p, int n, int Hi, int Wi, const int32_t* w) {
    return MetImg{p, n == 1 ? (int64_t)0 : (int64_t)Hi * Wi * 3, Wi, w[0], w[1]};
}
inline int64_t met_range_bytes(int N, int ref_n) { return (int64_t)(N + ref_n) * kMetSlices * 2 * (int64_t)sizeof(float); }   // met_range_kernel's output
}  // namespace

extern "C" int64_t pcdm_metrics_ws_bytes(int N, int ref_n, int W, int H, float sigma) {
    if (N <= 0 || N > 65535 || (ref_n != 1 && ref_n != N) || W <= 0 || H <= 0) return -1;
    int64_t bytes = met_range_bytes(N, ref_n);   // (pcdm_psnr: N * kMetSlices doubles, never more than this)
    if (sigma > 0.f) {
        const int r = ssim_radius(sigma);
        if (r < 1 || r > kSsimMaxR || W < 2 * r + 1 || H < 2 * r + 1) return -1;
        const int64_t tiles = (int64_t)((W - 2 * r + kSsimTW - 1) / kSsimTW) * ((H - 2 * r + kSsimTH - 1) / kSsimTH);
        bytes += (int64_t)N * tiles * sizeof(double);
    }
    return bytes;
}

extern "C" int pcdm_ssim(const void* cand, int N, int Hc, int Wc, const int32_t* cand_win, const void* ref, int ref_n, int Hr, int Wr,
                         const int32_t* ref_win, int channels, int is_f32, float sigma, float data_range, float* scores, int32_t* argmax,
                         void* ws, int64_t ws_bytes, pcdm_stream_t s) {
    if (!met_args_ok(cand, N, Hc, Wc, cand_win, ref, ref_n, Hr, Wr, ref_win, channels) || !scores || !ws || ((uintptr_t)ws & 7)) return -1;
    const int W = cand_win[2], H = cand_win[3], r = ssim_radius(sigma);
    if (r < 1 || r > kSsimMaxR || W < 2 * r + 1 || H < 2 * r + 1) return -1;
    if (ws_bytes < pcdm_metrics_ws_bytes(N, ref_n, W, H, sigma)) return -1;
    SsimTaps taps;
    double sum = 0.0;
    for (int k = 0; k <= 2 * r; ++k) sum += taps.w[k] = exp(-0.5 * ((double)(k - r) / (double)sigma) * ((double)(k - r) / (double)sigma));
    for (int k = 0; k <= 2 * kSsimMaxR; ++k) taps.w[k] = k <= 2 * r ? taps.w[k] / sum : 0.0;
    const MetImg ci = met_img(cand, 0, Hc, Wc, cand_win), ri = met_img(ref, ref_n, Hr, Wr, ref_win);
    float* ws_range = (float*)ws;
    double* ws_part = (double*)((char*)ws + met_range_bytes(N, ref_n));
    const int gx = (W - 2 * r + kSsimTW - 1) / kSsimTW, gy = (H - 2 * r + kSsimTH - 1) / kSsimTH;
    const int smem_max = 6 * (kSsimTH + 2 * kSsimMaxR) * (kSsimTW + 2 * kSsimMaxR) * (int)sizeof(float) +
                         5 * (kSsimTH + 2 * kSsimMaxR) * kSsimTW * (int)sizeof(double);
    const int smem = 6 * (kSsimTH + 2 * r) * (kSsimTW + 2 * r) * (int)sizeof(float) + 5 * (kSsimTH + 2 * r) * kSsimTW * (int)sizeof(double);
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)ssim_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, smem_max);
        attr_done = true;
    }
    PCDM_LAUNCH(met_range_kernel, dim3(kMetSlices, N + ref_n), dim3(256), 0, (hipStream_t)s, ci, ri, N, is_f32, W, H, ws_range);
    PCDM_CHECK_LAUNCH();
    PCDM_LAUNCH(ssim_tile_kernel, dim3(gx, gy, N), dim3(256), smem, (hipStream_t)s, ci, ri, N, is_f32, W, H, r, taps, data_range, ws_range, ws_part);
    PCDM_CHECK_LAUNCH();
    PCDM_LAUNCH(ssim_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, ws_part, N, gx * gy, 1.0 / (3.0 * (double)(W - 2 * r) * (double)(H - 2 * r)),
                scores, argmax);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_psnr(const void* cand, int N, int Hc, int Wc, const int32_t* cand_win, const void* ref, int ref_n, int Hr, int Wr,
                         const int32_t* ref_win, int channels, int is_f32, float data_range, float* mse, float* psnr, void* ws, int64_t ws_bytes,
                         pcdm_stream_t s) {
    if (!met_args_ok(cand, N, Hc, Wc, cand_win, ref, ref_n, Hr, Wr, ref_win, channels) || (!mse && !psnr) || !ws || ((uintptr_t)ws & 7)) return -1;
    const int W = cand_win[2], H = cand_win[3];
    if (!(data_range > 0.f) || ws_bytes < pcdm_metrics_ws_bytes(N, ref_n, W, H, 0.f)) return -1;
    const MetImg ci = met_img(cand, 0, Hc, Wc, cand_win), ri = met_img(ref, ref_n, Hr, Wr, ref_win);
    PCDM_LAUNCH(met_sqerr_kernel, dim3(kMetSlices, N), dim3(256), 0, (hipStream_t)s, ci, ri, is_f32, W, H, (double*)ws);
    PCDM_CHECK_LAUNCH();
    PCDM_LAUNCH(psnr_final_kernel, grid1d(N, 64), dim3(64), 0, (hipStream_t)s, (const double*)ws, N, 1.0 / (3.0 * (double)W * (double)H),
                (double)data_range, mse, psnr);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_select_image(const void* cand_u8, int N, int Hc, int Wc, const int32_t* win, int channels, const int32_t* index_dev, void* out,
                                 int normalized, pcdm_stream_t s) {
    if (!cand_u8 || N <= 0 || channels != 3 || !met_window_ok(Hc, Wc, win) || !index_dev || !out || (int64_t)win[2] * win[3] * 3 >= (int64_t)1 << 31) return -1;
    PCDM_LAUNCH(select_image_kernel, grid1d((int64_t)win[2] * win[3] * 3, 256), dim3(256), 0, (hipStream_t)s, (const uint8_t*)cand_u8, N, Hc, Wc,
                win[0], win[1], win[2], win[3], index_dev, out, normalized);
    PCDM_CHECK_LAUNCH();
    return 0;
}

// ---- the reference's metric scripts (metrics.py: calculate_from_disk; their OpenCV-cubic resize: image_prep.hip): L1 / MAE, and the uniform-window
// SSIM with the sample covariance ---------------------------------------------------------------------------------------------------------------
namespace {
constexpr int kAdSlices = 16;                   // 2 doubles per slice: N * 256 bytes, within pcdm_metrics_ws_bytes(..., sigma = 0)
constexpr int kBoxT = 16;                       // output tile (square) of ssim_box_tile_kernel
constexpr int kBoxMaxP = 25;                    // widest window: win_size = 2 * 25 + 1
__host__ __device__ inline int box_smem_bytes(int p) {
    const int T = kBoxT + 2 * p;
    return 2 * T * T * (int)sizeof(float) + 5 * T * kBoxT * (int)sizeof(double);
}

// ws_ad[(n * kAdSlices + slice) * 2] = {sum |a - b|, sum (a + b)} over the slice's rows: a - b and a + b in fp32 as numpy forms them on float32
// arrays, accumulated in fp64; uint8 inputs in integers (exact)
__global__ __launch_bounds__(256) void met_absdiff_kernel(MetImg cand, MetImg ref, int f32, int W, int H, double* __restrict__ ws_ad) {
    __shared__ double red[2][4];
    const int n = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x;
    const int rows = (H + kAdSlices - 1) / kAdSlices;
    const int ya = sl * rows, yb = imin(H, ya + rows);
    unsigned long long si0 = 0, si1 = 0;
    double sd0 = 0.0, sd1 = 0.0;
    for (int y = ya; y < yb; ++y)
        for (int x3 = tid; x3 < 3 * W; x3 += 256) {
            const float a = met_load(cand, f32, n, y, x3), b = met_load(ref, f32, n, y, x3);
            if (f32) {
                sd0 += (double)fabsf(a - b);
                sd1 += (double)(a + b);
            } else {
                const int d = (int)a - (int)b;
                si0 += (unsigned long long)(d < 0 ? -d : d);
                si1 += (unsigned long long)((int)a + (int)b);
            }
        }
    const double s0 = wave_sum_f64(f32 ? sd0 : (double)si0), s1 = wave_sum_f64(f32 ? sd1 : (double)si1);
    if ((tid & 63) == 0) { red[0][tid >> 6] = s0; red[1][tid >> 6] = s1; }
    __syncthreads();
    if (tid == 0) {
        ws_ad[(n * kAdSlices + sl) * 2 + 0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        ws_ad[(n * kAdSlices + sl) * 2 + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

__global__ void absdiff_final_kernel(const double* __restrict__ ws_ad, int N, double count, float* __restrict__ l1_out, float* __restrict__ mae_out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s0 = 0.0, s1 = 0.0;
    for (int i = 0; i < kAdSlices; ++i) {
        s0 += ws_ad[(n * kAdSlices + i) * 2];
        s1 += ws_ad[(n * kAdSlices + i) * 2 + 1];
    }
    if (l1_out) l1_out[n] = (float)(s0 / count);
    if (mae_out) mae_out[n] = (float)(s0 / s1);      // (0 / 0: NaN, x / 0: inf, as numpy divides)
}

// skimage.metrics.structural_similarity with its default uniform window (win_size = w = 2p + 1) and sample covariance: one workgroup per
// (candidate, 16 x 16 output tile), one channel at a time.  LDS: the (16 + 2p)^2 halo tile of both images, centred fp32 as in ssim_tile_kernel
// (8 (16 + 2p)^2 bytes), and the row sums of the five moments in fp64 (5 * 8 * 16 (16 + 2p) bytes): 77.1 KB at w = 51.  The window sums are plain
// fp64 sums of the w taps per axis, divided by NP = w^2 once; covariances times NP / (NP - 1).
__global__ __launch_bounds__(256) void ssim_box_tile_kernel(MetImg cand, MetImg ref, int N, int f32, int W, int H, int p, float data_range,
                                                            const float* __restrict__ ws_range, double* __restrict__ ws_part) {
    PCDM_DYN_SMEM(smem);
    __shared__ float s_rng[4];     // candidate min, max; reference min, max
    __shared__ double s_red[4];
    const int n = blockIdx.z, tid = threadIdx.x;
    const int T = kBoxT + 2 * p, w = 2 * p + 1;
    float* tile = (float*)smem;                                              // [2][T][T]
    double* hb = (double*)(smem + (size_t)2 * T * T * sizeof(float));        // [5][T][kBoxT]
    if (tid < 64) {
        const int which = tid >> 5, sl = tid & 31;
        const int img = which ? N + (ref.img_stride ? n : 0) : n;
        float mn = ws_range[(img * kMetSlices + sl) * 2], mx = ws_range[(img * kMetSlices + sl) * 2 + 1];
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, m, 64));
            mx = fmaxf(mx, __shfl_xor(mx, m, 64));
        }
        if (sl == 0) { s_rng[which * 2] = mn; s_rng[which * 2 + 1] = mx; }
    }
    __syncthreads();
    const float ca = 0.5f * (s_rng[0] + s_rng[1]), cb = 0.5f * (s_rng[2] + s_rng[3]);
    const double R = data_range >= 0.f ? (double)data_range : (double)s_rng[1] - (double)s_rng[0];
    const double c1 = (0.01 * R) * (0.01 * R), c2 = (0.03 * R) * (0.03 * R);
    const double np = (double)w * (double)w, inv_np = 1.0 / np, cov_norm = np / (np - 1.0);
    const int tx0 = blockIdx.x * kBoxT, ty0 = blockIdx.y * kBoxT;            // window coordinates of the halo tile's corner
    double acc = 0.0;
    for (int c = 0; c < 3; ++c) {
        for (int i = tid; i < T * T; i += 256) {
            const int row = i / T, px = i - row * T;
            const int gy = imin(ty0 + row, H - 1), gx = imin(tx0 + px, W - 1);   // (clamped: only tiles cut by the window's edge, outputs masked below)
            tile[row * T + px] = met_load(cand, f32, n, gy, gx * 3 + c) - ca;
            tile[(T + row) * T + px] = met_load(ref, f32, n, gy, gx * 3 + c) - cb;
        }
        __syncthreads();
        for (int o = tid; o < T * kBoxT; o += 256) {                 // rows: sums of x, y, xx, yy, xy of the centred values over w columns
            const int row = o / kBoxT, col = o - row * kBoxT;
            double m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0;
            for (int k = 0; k < w; ++k) {
                const double x = tile[row * T + col + k], y = tile[(T + row) * T + col + k];
                m0 += x; m1 += y; m2 += x * x; m3 += y * y; m4 += x * y;
            }
            hb[(0 * T + row) * kBoxT + col] = m0;
            hb[(1 * T + row) * kBoxT + col] = m1;
            hb[(2 * T + row) * kBoxT + col] = m2;
            hb[(3 * T + row) * kBoxT + col] = m3;
            hb[(4 * T + row) * kBoxT + col] = m4;
        }
        __syncthreads();
        {                                                            // columns (one output pixel per lane), then the SSIM map
            const int row = tid / kBoxT, col = tid - row * kBoxT;
            double m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0;
            for (int k = 0; k < w; ++k) {
                m0 += hb[(0 * T + row + k) * kBoxT + col];
                m1 += hb[(1 * T + row + k) * kBoxT + col];
                m2 += hb[(2 * T + row + k) * kBoxT + col];
                m3 += hb[(3 * T + row + k) * kBoxT + col];
                m4 += hb[(4 * T + row + k) * kBoxT + col];
            }
            if (tx0 + p + col < W - p && ty0 + p + row < H - p) {
                m0 *= inv_np; m1 *= inv_np; m2 *= inv_np; m3 *= inv_np; m4 *= inv_np;
                const double ux = m0 + (double)ca, uy = m1 + (double)cb;
                const double vx = cov_norm * (m2 - m0 * m0), vy = cov_norm * (m3 - m1 * m1), vxy = cov_norm * (m4 - m0 * m1);
                acc += ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
            }
        }
        __syncthreads();
    }
    acc = wave_sum_f64(acc);
    if ((tid & 63) == 0) s_red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0)
        ws_part[((int64_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}
}  // namespace

extern "C" int pcdm_absdiff(const void* cand, int N, int Hc, int Wc, const int32_t* cand_win, const void* ref, int ref_n, int Hr, int Wr,
                            const int32_t* ref_win, int channels, int is_f32, float* l1, float* mae, void* ws, int64_t ws_bytes, pcdm_stream_t s) {
    if (!met_args_ok(cand, N, Hc, Wc, cand_win, ref, ref_n, Hr, Wr, ref_win, channels) || (!l1 && !mae) || !ws || ((uintptr_t)ws & 7)) return -1;
    const int W = cand_win[2], H = cand_win[3];
    if (ws_bytes < pcdm_metrics_ws_bytes(N, ref_n, W, H, 0.f)) return -1;     // (N * kAdSlices * 2 doubles = N * 256 bytes: never more than that)
    const MetImg ci = met_img(cand, 0, Hc, Wc, cand_win), ri = met_img(ref, ref_n, Hr, Wr, ref_win);
    PCDM_LAUNCH(met_absdiff_kernel, dim3(kAdSlices, N), dim3(256), 0, (hipStream_t)s, ci, ri, is_f32, W, H, (double*)ws);
    PCDM_CHECK_LAUNCH();
    PCDM_LAUNCH(absdiff_final_kernel, grid1d(N, 64), dim3(64), 0, (hipStream_t)s, (const double*)ws, N, 3.0 * (double)W * (double)H, l1, mae);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t pcdm_ssim_box_ws_bytes(int N, int ref_n, int W, int H, int win_size) {
    if (N <= 0 || N > 65535 || (ref_n != 1 && ref_n != N) || W <= 0 || H <= 0) return -1;
    if (win_size < 3 || win_size > 2 * kBoxMaxP + 1 || !(win_size & 1) || W < win_size || H < win_size) return -1;
    const int64_t tiles = (int64_t)((W - win_size + 1 + kBoxT - 1) / kBoxT) * ((H - win_size + 1 + kBoxT - 1) / kBoxT);
    return met_range_bytes(N, ref_n) + (int64_t)N * tiles * sizeof(double);
}

extern "C" int pcdm_ssim_box(const void* cand, int N, int Hc, int Wc, const int32_t* cand_win, const void* ref, int ref_n, int Hr, int Wr,
                             const int32_t* ref_win, int channels, int is_f32, int win_size, float data_range, float* scores, void* ws,
                             int64_t ws_bytes, pcdm_stream_t s) {
    if (!met_args_ok(cand, N, Hc, Wc, cand_win, ref, ref_n, Hr, Wr, ref_win, channels) || !scores || !ws || ((uintptr_t)ws & 7)) return -1;
    const int W = cand_win[2], H = cand_win[3];
    const int64_t need = pcdm_ssim_box_ws_bytes(N, ref_n, W, H, win_size);
    if (need < 0 || ws_bytes < need) return -1;
    const int p = (win_size - 1) / 2;
    const int gx = (W - 2 * p + kBoxT - 1) / kBoxT, gy = (H - 2 * p + kBoxT - 1) / kBoxT;
    if (gy > 65535) return -1;
    const MetImg ci = met_img(cand, 0, Hc, Wc, cand_win), ri = met_img(ref, ref_n, Hr, Wr, ref_win);
    float* ws_range = (float*)ws;
    double* ws_part = (double*)((char*)ws + met_range_bytes(N, ref_n));
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)ssim_box_tile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, box_smem_bytes(kBoxMaxP));
        attr_done = true;
    }
    PCDM_LAUNCH(met_range_kernel, dim3(kMetSlices, N + ref_n), dim3(256), 0, (hipStream_t)s, ci, ri, N, is_f32, W, H, ws_range);
    PCDM_CHECK_LAUNCH();
    PCDM_LAUNCH(ssim_box_tile_kernel, dim3(gx, gy, N), dim3(256), box_smem_bytes(p), (hipStream_t)s, ci, ri, N, is_f32, W, H, p, data_range, ws_range,
                ws_part);
    PCDM_CHECK_LAUNCH();
    PCDM_LAUNCH(ssim_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, ws_part, N, gx * gy, 1.0 / (3.0 * (double)(W - 2 * p) * (double)(H - 2 * p)),
                scores, (int32_t*)nullptr);
    PCDM_CHECK_LAUNCH();
    return 0;
}
