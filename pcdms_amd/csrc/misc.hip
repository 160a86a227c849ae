// Small / elementwise kernels of the stage-2 denoise step (SURVEY.md §2.1 K12, K13 and the
// input assembly of stage2_inpaint_pipeline.py:499-501).  All HBM- or latency-bound; 16-byte
// vector accesses where the layout allows, device-resident step index so one captured hipGraph
// replays for every timestep.
#include "pcdm_device.h"
#include "../../include/pcdm.h"

namespace {
// out[b, j]: diffusers Timesteps (flip_sin_to_cos => [cos | sin])
__global__ void timestep_embedding_kernel(const int64_t* __restrict__ t_dev, const int32_t* __restrict__ step_dev,
                                          float* __restrict__ out, int B, int dim, int flip, float shift) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * dim) return;
    const int j = i % dim, half = dim / 2;
    const float tv = (float)t_dev[step_dev ? *step_dev : 0];
    const int kk = j < half ? j : j - half;
    const float f = expf(-9.210340371976184f * (float)kk / ((float)half - shift));
    const float a = tv * f;
    const bool is_cos = flip ? (j < half) : (j >= half);
    out[i] = is_cos ? cosf(a) : sinf(a);
}

// the same for a table of timesteps: row i <- t_dev[i]
__global__ void timestep_embedding_rows_kernel(const int64_t* __restrict__ t_dev, float* __restrict__ out, int n, int dim, int flip, float shift) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * dim) return;
    const int j = i % dim, half = dim / 2;
    const float tv = (float)t_dev[i / dim];
    const int kk = j < half ? j : j - half;
    const float f = expf(-9.210340371976184f * (float)kk / ((float)half - shift));
    const float a = tv * f;
    const bool is_cos = flip ? (j < half) : (j >= half);
    out[i] = is_cos ? cosf(a) : sinf(a);
}

// out[(i * B + b) * D + d] = bf16( silu( emb_t[i * D + d] + cls[b * D + d] ) )   (cls may be NULL)
__global__ void time_class_combine_kernel(const float* __restrict__ emb_t, const float* __restrict__ cls, u16* __restrict__ out, int n, int B, int D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * B * D) return;
    const int d = (int)(i % D);
    const int64_t r = i / D;
    const int b = (int)(r % B), st = (int)(r / B);
    float v = emb_t[(int64_t)st * D + d];
    if (cls) v += cls[(int64_t)b * D + d];
    out[i] = f2bf(silu_f(v));
}

// y[b, n] = act_out( sum_k act_in(x[b,k]) W[n,k] + bias[n] ) + add[b,n]; one wave per n.
__global__ __launch_bounds__(256) void small_linear_kernel(const float* __restrict__ x, const u16* __restrict__ w,
                                                           const float* __restrict__ bias,
                                                           const float* __restrict__ add, float* __restrict__ y,
                                                           int B, int K, int N, int act_in, int act_out) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool valid = n < N;
    const u16* wr = w + (int64_t)(valid ? n : 0) * K;
    for (int b0 = 0; b0 < B; b0 += 8) {
        float acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = 0.f;
        for (int k = lane * 8; k < K; k += 64 * 8) {
            const u16x8 wv = *(const u16x8*)(wr + k);
            float wf[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) wf[e] = bf2f(wv[e]);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (b0 + i < B) {
                    const float* xr = x + (int64_t)(b0 + i) * K + k;
                    const f32x4 x0 = *(const f32x4*)xr, x1 = *(const f32x4*)(xr + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float a0 = x0[e], a1 = x1[e];
                        if (act_in) {
                            a0 = silu_f(a0);
                            a1 = silu_f(a1);
                        }
                        acc[i] += a0 * wf[e] + a1 * wf[e + 4];
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float s = wave_sum(acc[i]);
            if (lane == 0 && valid && b0 + i < B) {
                float v = s + (bias ? bias[n] : 0.f);
                if (act_out == 1) v = silu_f(v);
                if (add) v += add[(int64_t)(b0 + i) * N + n];
                if (act_out == 2) v = silu_f(v);   // activation of the SUM (emb = time + class, consumed as silu(emb))
                y[(int64_t)(b0 + i) * N + n] = v;
            }
        }
    }
}

__global__ void assemble_input_kernel(const float* __restrict__ latents, int N, int rep,
                                      const float* __restrict__ mask, int mask_b, const float* __restrict__ masked,
                                      int masked_b, u16* __restrict__ out, int HW, int cpad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (b, pixel, octet)
    const int noct = cpad / 8;
    const int64_t total = (int64_t)N * rep * HW * noct;
    if (i >= total) return;
    const int oc = (int)(i % noct);
    const int64_t bp = i / noct;
    const int pix = (int)(bp % HW), b = (int)(bp / HW);
    u16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = oc * 8 + e;
        float v = 0.f;
        const int c0 = mask ? 5 : 4;   // no mask channel: [latents | masked] (the stage-3 refinement input)
        if (c < 4) v = latents[((int64_t)(b % N) * 4 + c) * HW + pix];
        else if (mask && c == 4) v = mask[(int64_t)(mask_b == 1 ? 0 : b) * HW + pix];
        else if (c >= c0 && c < c0 + 4) v = masked[((int64_t)(masked_b == 1 ? 0 : b) * 4 + (c - c0)) * HW + pix];
        o[e] = f2bf(v);
    }
    *(u16x8*)(out + i * 8) = o;
}

__global__ void nchw_to_nhwc_kernel(const float* __restrict__ x, u16* __restrict__ y, int C, int Cpad, int HW,
                                    int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (b, pixel, octet)
    if (i >= total) return;
    const int noct = Cpad / 8;
    const int oc = (int)(i % noct);
    const int64_t bp = i / noct;
    const int pix = (int)(bp % HW);
    const int64_t b = bp / HW;
    u16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = oc * 8 + e;
        o[e] = c < C ? f2bf(x[(b * C + c) * HW + pix]) : (u16)0;
    }
    *(u16x8*)(y + i * 8) = o;
}

__global__ void nhwc_to_nchw_kernel(const u16* __restrict__ x, float* __restrict__ y, int C, int HW, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over (b, c, pix)
    if (i >= total) return;
    const int pix = (int)(i % HW);
    const int64_t bc = i / HW;
    const int c = (int)(bc % C);
    const int64_t b = bc / C;
    y[i] = bf2f(x[(b * HW + pix) * C + c]);
}

__global__ void f32_to_bf16_kernel(const float* __restrict__ x, u16* __restrict__ y, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = f2bf(x[i]);
}

__global__ void cfg_step_kernel(const float* __restrict__ eps, int cfg, float g, const float* __restrict__ x,
                                const float* __restrict__ noise, float* __restrict__ x_prev,
                                float* __restrict__ eps_out, const float* __restrict__ coef,
                                const int32_t* __restrict__ step_dev, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* cf = coef + 4 * (step_dev ? *step_dev : 0);
    float e = eps[i];
    if (cfg) e = e + g * (eps[n + i] - e);
    if (eps_out) eps_out[i] = e;
    if (x_prev) {
        float v = cf[0] * x[i] + cf[1] * e;
        if (noise) v += cf[2] * noise[i];
        x_prev[i] = v;
    }
}

// UniPCMultistepScheduler.step (order <= 2, predict_x0, bh1 / bh2) as ONE elementwise kernel on static
// state slots, so the whole UniPC update is graph-replayable: the step's twelve host-computed scalars come from a DEVICE table
// row selected by the device step counter.
//   m_t   = c[0] x + c[1] eps                                   (x0-prediction, convert_model_output)
//   x_c   = c[2] != 0 ? c[3] last + c[4] m1 + c[5] m2 + c[6] m_t : x     (corrector; m1 = newest stored output, m2 the one before)
//   x'    = c[7] x_c + c[8] m_t + c[9] m1                        (predictor, after the history shift m_t -> m1 -> m2)
// and the state advances in place: x <- x', m2 <- m1, m1 <- m_t, last <- x_c.  Every element is owned by one thread.
__global__ void unipc_step_kernel(const float* __restrict__ eps, int cfg, float g, float* __restrict__ x, float* __restrict__ m1,
                                  float* __restrict__ m2, float* __restrict__ last, const float* __restrict__ coef,
                                  const int32_t* __restrict__ step_dev, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* c = coef + 12 * (step_dev ? *step_dev : 0);
    float e = eps[i];
    if (cfg) e = e + g * (eps[n + i] - e);
    const float xi = x[i], a1 = m1[i], a2 = m2[i];
    const float mt = c[0] * xi + c[1] * e;
    float xc = xi;
    if (c[2] != 0.f) xc = c[3] * last[i] + c[4] * a1 + c[5] * a2 + c[6] * mt;
    x[i] = c[7] * xc + c[8] * mt + c[9] * a1;
    m2[i] = a1;
    m1[i] = mt;
    last[i] = xc;
}

// DPMSolverMultistepScheduler.step (dpmsolver++ / sde-dpmsolver++, order <= 2, midpoint / heun) as ONE elementwise kernel on one
// static history slot: every variant is linear in (x, eps, m1, noise) with host-known scalars, row *step_dev of a DEVICE table
// c = {a_x, a_e, p_x, p_m0, p_m1, p_z, 0, 0}:
//   m0 = a_x x + a_e eps                                        (x0-prediction, convert_model_output)
//   x' = p_x x + p_m0 m0 + p_m1 m1 + p_z noise_all[*step_dev, i] (noise_all NULL: no noise term)
// then, in place: x <- x', m1 <- m0.  Every element is owned by one thread.
__global__ void dpmpp_step_kernel(const float* __restrict__ eps, int cfg, float g, float* __restrict__ x, float* __restrict__ m1,
                                  const float* __restrict__ noise_all, const float* __restrict__ coef,
                                  const int32_t* __restrict__ step_dev, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int st = step_dev ? *step_dev : 0;
    const float* c = coef + 8 * st;
    float e = eps[i];
    if (cfg) e = e + g * (eps[n + i] - e);
    const float xi = x[i];
    const float m0 = c[0] * xi + c[1] * e;
    float v = c[2] * xi + c[3] * m0 + c[4] * m1[i];
    if (noise_all) v += c[5] * noise_all[(int64_t)st * n + i];
    x[i] = v;
    m1[i] = m0;
}

// UnCLIPScheduler.step on a [N, n/N] vector (stage-1 prior): guided prediction -> x0 -> clip -> posterior mean (+ noise),
// then an optional affine read-out (post_process_latents).  c = {p_x, p_e, clip, c_x0, c_x, c_noise, out_scale, out_shift}.
struct UnclipArgs { float c[8]; };
__global__ void unclip_step_kernel(const float* __restrict__ pred, int cfg, float g, const float* __restrict__ x,
                                   const float* __restrict__ noise, float* __restrict__ x_prev, UnclipArgs a, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float e = pred[i];
    if (cfg) e = e + g * (pred[n + i] - e);
    const float xi = x[i];
    float x0 = a.c[0] * xi + a.c[1] * e;
    if (a.c[2] > 0.f) x0 = fminf(fmaxf(x0, -a.c[2]), a.c[2]);
    float v = a.c[3] * x0 + a.c[4] * xi;
    if (noise) v += a.c[5] * noise[i];
    x_prev[i] = v * a.c[6] + a.c[7];
}

// the same with the step's eight coefficients and its noise slab taken from DEVICE tables at *step_dev (hipGraph-replayable stage-1 loop)
__global__ void unclip_step_dev_kernel(const float* __restrict__ pred, int cfg, float g, float* __restrict__ x,
                                       const float* __restrict__ noise_all, const float* __restrict__ coef,
                                       const int32_t* __restrict__ step_dev, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int st = *step_dev;
    const float* c = coef + 8 * st;
    float e = pred[i];
    if (cfg) e = e + g * (pred[n + i] - e);
    const float xi = x[i];
    float x0 = c[0] * xi + c[1] * e;
    if (c[2] > 0.f) x0 = fminf(fmaxf(x0, -c[2]), c[2]);
    float v = c[3] * x0 + c[4] * xi;
    if (noise_all && c[5] != 0.f) v += c[5] * noise_all[(int64_t)st * n + i];
    x[i] = v * c[6] + c[7];
}

struct LinArgs {
    const float* x[6];
    float c[6];
};
__global__ void lincomb_kernel(float* __restrict__ y, int nin, LinArgs a, const float* __restrict__ cdev, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = 0.f;
    for (int j = 0; j < nin; ++j) v += (cdev ? cdev[j] : a.c[j]) * a.x[j][i];
    y[i] = v;
}

// rescale_noise_cfg (ref stage2_inpaint_pipeline.py:52-63): per-sample unbiased std of the guided eps and of the
// conditional eps over all C*H*W elements; out = gr * cfg * (std_text / std_cfg) + (1 - gr) * cfg.
// One workgroup per sample; fp64 block reduction (wave64 shuffles + LDS).
__global__ __launch_bounds__(1024) void rescale_cfg_kernel(const float* __restrict__ cfg_eps,
                                                           const float* __restrict__ text_eps, float* __restrict__ out,
                                                           int64_t n, float gr) {
    __shared__ double red[16][4];
    __shared__ float factor;
    const float* a = cfg_eps + (int64_t)blockIdx.x * n;
    const float* b = text_eps + (int64_t)blockIdx.x * n;
    double s[4] = {0, 0, 0, 0};
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        const double x = a[i], y = b[i];
        s[0] += x; s[1] += x * x; s[2] += y; s[3] += y * y;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s[k] += __shfl_xor(s[k], m, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
        for (int k = 0; k < 4; ++k) red[wave][k] = s[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4] = {0, 0, 0, 0};
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w)
            for (int k = 0; k < 4; ++k) t[k] += red[w][k];
        const double var_c = (t[1] - t[0] * t[0] / (double)n) / (double)(n - 1);
        const double var_t = (t[3] - t[2] * t[2] / (double)n) / (double)(n - 1);
        factor = (float)sqrt(var_t / var_c);
    }
    __syncthreads();
    const float f = gr * factor + (1.0f - gr);
    float* o = out + (int64_t)blockIdx.x * n;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) o[i] = a[i] * f;
}

// p[r, :] = softmax(scale * s[r, :]) as bf16; one workgroup (256 threads) per row, the row lives in registers
// (cols <= 8192), fp32 max / exp / sum with wave64 shuffles + LDS across the 4 waves.  Used by the VAE's single-head
// d=512 attention (two MFMA GEMMs around it), SURVEY.md §8f N1.
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ s, u16* __restrict__ p, int cols,
                                                           int64_t ld_s, int64_t ld_p, float scale_log2e) {
    __shared__ float red[4];
    const float* sr = s + (int64_t)blockIdx.x * ld_s;
    u16* pr = p + (int64_t)blockIdx.x * ld_p;
    const int t = threadIdx.x;
    float v[32];
    float mx = -1e30f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const int c = t + 256 * i;
        v[i] = c < cols ? sr[c] * scale_log2e : -1e30f;
        mx = fmaxf(mx, v[i]);
    }
    mx = wave_max(mx);
    if ((t & 63) == 0) red[t >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        v[i] = fast_exp2(v[i] - mx);
        sum += (t + 256 * i < cols) ? v[i] : 0.f;
    }
    sum = wave_sum(sum);
    if ((t & 63) == 0) red[t >> 6] = sum;
    __syncthreads();
    const float inv = 1.0f / (red[0] + red[1] + red[2] + red[3]);
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const int c = t + 256 * i;
        if (c < cols) pr[c] = f2bf(v[i] * inv);
    }
}

// DiagonalGaussianDistribution.sample() * scaling_factor (ref stage2_inpaint_pipeline.py:443-444):
// moments fp32 [B, 2*zc, HW] (mean | logvar); out = (mean + exp(0.5*clamp(logvar,-30,20)) * noise) * scale
__global__ void gaussian_sample_kernel(const float* __restrict__ mom, const float* __restrict__ noise,
                                       float* __restrict__ out, int zc, int HW, float scale, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over (b, c, pix)
    if (i >= total) return;
    const int64_t chw = (int64_t)zc * HW;
    const int64_t b = i / chw, r = i - b * chw;
    const float mean = mom[b * 2 * chw + r];
    float lv = mom[b * 2 * chw + chw + r];
    lv = fminf(fmaxf(lv, -30.0f), 20.0f);
    const float z = noise ? noise[i] : 0.f;
    out[i] = (mean + __expf(0.5f * lv) * z) * scale;
}

// VaeImageProcessor.postprocess: (x/2+0.5).clamp(0,1) -> NHWC -> round(255 x) -> uint8.  x fp32 [B, cstride>=3, HW] (NCHW)
__global__ void image_to_uint8_kernel(const float* __restrict__ x, uint8_t* __restrict__ out, int cstride, int HW,
                                      int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over (b, pix)
    if (i >= total) return;
    const int64_t b = i / HW, pix = i - b * HW;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = x[(b * cstride + c) * HW + pix] * 0.5f + 0.5f;
        v = fminf(fmaxf(v, 0.f), 1.f);
        out[i * 3 + c] = (uint8_t)rintf(v * 255.0f);
    }
}

// out NHWC [B, 2H, 2W, C] <- in [B H W, 4 C] (phase 2a + b major): the pixel shuffle behind the phase-decomposed Upsample2D convolution.
// One thread per 16 bytes of output: consecutive threads walk the channels of one output pixel, then the next pixel of the output row.
__global__ void pixel_shuffle2_kernel(const u16* __restrict__ in, u16* __restrict__ out, int H, int W, int C8, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c8 = (int)(i % C8);
    const int64_t px = i / C8;                  // output pixel index (b, Y, X)
    const int W2 = 2 * W;
    const int X = (int)(px % W2);
    const int64_t bY = px / W2;                 // b * 2H + Y
    const int Y = (int)(bY % (2 * H));
    const int64_t b = bY / (2 * H);
    const int64_t src = (((b * H + (Y >> 1)) * W + (X >> 1)) * 4 + ((Y & 1) * 2 + (X & 1))) * C8 + c8;
    ((u32x4*)out)[i] = ((const u32x4*)in)[src];
}

// ---- image metrics of the evaluation drivers (stage2_batchtest_inpaint_model.py:203-219: the best-of-N pick by Gaussian-weighted SSIM) ---------
// A batch of N candidates against one reference (or one per candidate), each a WINDOW (x0, y0, W, H) into uint8 / fp32 NHWC images with 3
// channels, scored where the decoder left them.  skimage.metrics.structural_similarity(gaussian_weights=True, use_sample_covariance=False):
// separable Gaussian of radius r = int(3.5 sigma + 0.5), five filtered moments per channel, SSIM map averaged over the interior
// [r, H - r) x [r, W - r) -- so every tap of every averaged pixel lies inside the window and the filter's boundary mode never enters.
// Numerics: both images are centred by the midpoint of their own min / max (met_range_kernel) before the second moments are formed -- the
// covariances do not depend on the shift, the means get it added back -- and the moments accumulate in fp64: a constant image gives exact
// zeros (so constant against constant is 0/0 = NaN for ANY constant, as the formula says), a near-constant one loses nothing to E[x^2] - mu^2.
// No atomics: per-workgroup partials in a caller-provided workspace, added per image in a fixed order by one last launch (bit-identical reruns).
constexpr int kMetSlices = 32;                  // row slices per image of the min / max and squared-error passes
constexpr int kSsimTW = 32, kSsimTH = 16;       // output tile of ssim_tile_kernel
constexpr int kSsimMaxR = 8;

struct MetImg {            // window into [n, Hi, Wi, 3]
    const void* p;
    int64_t img_stride;    // elements between images; 0: the same image for every candidate
    int Wi, x0, y0;
};
struct SsimTaps { double w[2 * kSsimMaxR + 1]; };
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

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

// the refusals shared by pcdm_ssim / pcdm_psnr (include/pcdm.h)
inline bool met_window_ok(int Hi, int Wi, const int32_t* w) {
    return w && Hi > 0 && Wi > 0 && w[0] >= 0 && w[1] >= 0 && w[2] > 0 && w[3] > 0 && (int64_t)w[0] + w[2] <= Wi && (int64_t)w[1] + w[3] <= Hi;
}
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

// ---- input preparation of the evaluation drivers (stage2_batchtest_inpaint_model.py:135-149: Image.resize(..., BICUBIC), canvas pasting,
// ToTensor + Normalize, CLIPImageProcessor) ------------------------------------------------------------------------------------------------
// Pillow's 8-bit resampler restated: per axis a table {lo[o], count[o], int32 coeff[o][k]} of 22-bit fixed-point weights (built on the host as
// Pillow builds them, include/pcdm.h), per output byte clip8((2^21 + sum coeff * pixel) >> 22) in 32-bit integers, the horizontal pass rounded to
// uint8 before the vertical pass reads it.  The kernels know nothing about the filter.  A table comes from the caller's device memory, so every
// entry is clamped into the image before it is used: a wrong table gives wrong pixels, never an access outside src, the LDS tile or the window.
constexpr int kRsTW = 32, kRsTH = 16;           // output tile of resample_tile_kernel
constexpr int kRsLdsBytes = 24 * 1024;          // most LDS one tile may ask for: 256 rows of 3 channels (6 workgroups a CU); beyond it: two launches
constexpr int kRsBits = 22;                     // Pillow's PRECISION_BITS for 8-bit images

struct RsAxis {            // tab == nullptr: the axis keeps its size and is copied (Pillow skips that pass)
    const int32_t* tab;    // [lo (n_out) | count (n_out) | coeff (n_out * k)]
    int n_out, k, n_in;
};
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
struct U8Norm { float mean[4], sd[4]; };
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

// ---- the reference's metric scripts (metrics.py: calculate_from_disk): OpenCV's INTER_CUBIC resize of float images, L1 / MAE, and the
// uniform-window SSIM with the sample covariance ------------------------------------------------------------------------------------------------------
// cv2.resize(float32 image, INTER_CUBIC) restated (resizeGeneric_ with HResizeCubic / VResizeCubic, float work type): per axis scale =
// 1 / (n_out / n_in) in double, f = float((d + 0.5) scale - 0.5), s = floor(f), t = f - s in fp32, taps s - 1 .. s + 2 clamped into the image, the
// Keys coefficients with A = -0.75 in fp32, the horizontal pass first.  No antialiasing, no rounding, no clipping.  Every fp32 / fp64 operation
// below is a separate IEEE operation (cv_mul): a fused multiply-add would round once where OpenCV's C++ rounds twice.
constexpr int kCvTW = 32, kCvTH = 16;           // output tile of resize_cubic_kernel
constexpr int kCvRows = 4 * kCvTH;              // LDS rows of a tile: a contiguous span of source rows, or four rows per output row

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

// ws_ad[(n * kAdSlices + slice) * 2] = {sum |a - b|, sum (a + b)} over the slice's rows: a - b and a + b in fp32 as numpy forms them on float32
// arrays, accumulated in fp64; uint8 inputs in integers (exact)
constexpr int kAdSlices = 16;                   // 2 doubles per slice: N * 256 bytes, within pcdm_metrics_ws_bytes(..., sigma = 0)
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
constexpr int kBoxT = 16;
constexpr int kBoxMaxP = 25;
__host__ __device__ inline int box_smem_bytes(int p) {
    const int T = kBoxT + 2 * p;
    return 2 * T * T * (int)sizeof(float) + 5 * T * kBoxT * (int)sizeof(double);
}
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

__global__ void advance_step_kernel(int32_t* step) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *step += 1;
}

inline dim3 grid1d(int64_t n, int bs) { return dim3((unsigned)((n + bs - 1) / bs)); }
}  // namespace

extern "C" int pcdm_version(void) { return PCDM_ABI_VERSION; }   // 5: pcdm_gemm_params starts with struct_size, ends with a3 / lda3 (include/pcdm.h)
extern "C" int pcdm_is_emulator(void) {
#ifdef PCDM_EMU
    return 1;
#else
    return 0;
#endif
}

extern "C" int pcdm_timestep_embedding(const int64_t* t_dev, const int32_t* step_dev, float* out, int B, int dim,
                                       int flip_sin_to_cos, float shift, pcdm_stream_t s) {
    if (!t_dev || !out || B <= 0 || dim <= 0 || dim % 2) return -1;
    PCDM_LAUNCH(timestep_embedding_kernel, grid1d((int64_t)B * dim, 256), dim3(256), 0, (hipStream_t)s, t_dev, step_dev,
                out, B, dim, flip_sin_to_cos, shift);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_timestep_embedding_rows(const int64_t* t_dev, int n, float* out, int dim, int flip_sin_to_cos, float shift, pcdm_stream_t s) {
    if (!t_dev || !out || n <= 0 || dim <= 0 || dim % 2) return -1;
    PCDM_LAUNCH(timestep_embedding_rows_kernel, grid1d((int64_t)n * dim, 256), dim3(256), 0, (hipStream_t)s, t_dev, out, n, dim, flip_sin_to_cos, shift);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_time_class_combine(const float* emb_t, const float* cls, void* out_bf16, int n, int B, int D, pcdm_stream_t s) {
    if (!emb_t || !out_bf16 || n <= 0 || B <= 0 || D <= 0) return -1;
    PCDM_LAUNCH(time_class_combine_kernel, grid1d((int64_t)n * B * D, 256), dim3(256), 0, (hipStream_t)s, emb_t, cls, (u16*)out_bf16, n, B, D);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_small_linear(const float* x, const void* w, const float* bias, const float* add, float* y, int B,
                                 int K, int N, int act_in, int act_out, pcdm_stream_t s) {
    if (!x || !w || !y || B <= 0 || B > 32 || K <= 0 || K % 8 || N <= 0) return -1;
    PCDM_LAUNCH(small_linear_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)s, x, (const u16*)w, bias, add, y,
                B, K, N, act_in, act_out);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_assemble_input(const float* latents, int N, int rep, const float* mask, int mask_b,
                                   const float* masked, int masked_b, void* out, int h, int w, int cpad,
                                   pcdm_stream_t s) {
    if (!latents || !masked || !out || N <= 0 || rep <= 0 || cpad % 8 || cpad < 16) return -1;   // mask == NULL: [latents | masked]
    const int64_t total = (int64_t)N * rep * h * w * (cpad / 8);
    PCDM_LAUNCH(assemble_input_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, latents, N, rep, mask, mask_b,
                masked, masked_b, (u16*)out, h * w, cpad);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_nchw_f32_to_nhwc_bf16(const float* x, void* y, int B, int C, int Cpad, int HW, pcdm_stream_t s) {
    if (!x || !y || Cpad % 8 || Cpad < C) return -1;
    const int64_t total = (int64_t)B * HW * (Cpad / 8);
    PCDM_LAUNCH(nchw_to_nhwc_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, x, (u16*)y, C, Cpad, HW, total);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_nhwc_bf16_to_nchw_f32(const void* x, float* y, int B, int C, int HW, pcdm_stream_t s) {
    if (!x || !y) return -1;
    const int64_t total = (int64_t)B * HW * C;
    PCDM_LAUNCH(nhwc_to_nchw_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, (const u16*)x, y, C, HW, total);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_f32_to_bf16(const float* x, void* y, int64_t n, pcdm_stream_t s) {
    if (!x || !y || n <= 0) return -1;
    PCDM_LAUNCH(f32_to_bf16_kernel, grid1d(n, 256), dim3(256), 0, (hipStream_t)s, x, (u16*)y, n);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_cfg_step(const float* eps, int cfg, float g, const float* x, const float* noise, float* x_prev,
                             float* eps_out, const float* coef, const int32_t* step_dev, int64_t n, pcdm_stream_t s) {
    if (!eps || n <= 0 || (x_prev && (!x || !coef))) return -1;
    PCDM_LAUNCH(cfg_step_kernel, grid1d(n, 256), dim3(256), 0, (hipStream_t)s, eps, cfg, g, x, noise, x_prev, eps_out,
                coef, step_dev, n);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_unipc_step(const float* eps, int cfg, float g, float* x, float* m1, float* m2, float* last, const float* coef,
                               const int32_t* step_dev, int64_t n, pcdm_stream_t s) {
    if (!eps || !x || !m1 || !m2 || !last || !coef || n <= 0) return -1;
    PCDM_LAUNCH(unipc_step_kernel, grid1d(n, 256), dim3(256), 0, (hipStream_t)s, eps, cfg, g, x, m1, m2, last, coef, step_dev, n);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_dpmpp_step(const float* eps, int cfg, float g, float* x, float* m1, const float* noise_all, const float* coef,
                               const int32_t* step_dev, int64_t n, pcdm_stream_t s) {
    if (!eps || !x || !m1 || !coef || n <= 0) return -1;
    PCDM_LAUNCH(dpmpp_step_kernel, grid1d(n, 256), dim3(256), 0, (hipStream_t)s, eps, cfg, g, x, m1, noise_all, coef, step_dev, n);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_unclip_step(const float* pred, int cfg, float g, const float* x, const float* noise, float* x_prev,
                                const float* c8, int64_t n, pcdm_stream_t s) {
    if (!pred || !x || !x_prev || !c8 || n <= 0) return -1;
    UnclipArgs a;
    for (int i = 0; i < 8; ++i) a.c[i] = c8[i];
    PCDM_LAUNCH(unclip_step_kernel, grid1d(n, 256), dim3(256), 0, (hipStream_t)s, pred, cfg, g, x, noise, x_prev, a, n);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_unclip_step_dev(const float* pred, int cfg, float g, float* x, const float* noise_all, const float* coef,
                                    const int32_t* step_dev, int64_t n, pcdm_stream_t s) {
    if (!pred || !x || !coef || !step_dev || n <= 0) return -1;
    PCDM_LAUNCH(unclip_step_dev_kernel, grid1d(n, 256), dim3(256), 0, (hipStream_t)s, pred, cfg, g, x, noise_all, coef, step_dev, n);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_lincomb(float* y, int nin, const float* const* xs, const float* c, int64_t n, pcdm_stream_t s) {
    if (!y || nin <= 0 || nin > 6 || !xs || !c || n <= 0) return -1;
    LinArgs a;
    for (int i = 0; i < 6; ++i) {
        a.x[i] = i < nin ? xs[i] : nullptr;
        a.c[i] = i < nin ? c[i] : 0.f;
    }
    PCDM_LAUNCH(lincomb_kernel, grid1d(n, 256), dim3(256), 0, (hipStream_t)s, y, nin, a, (const float*)nullptr, n);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_rescale_noise_cfg(const float* cfg_eps, const float* text_eps, float* out, int N, int64_t n,
                                      float guidance_rescale, pcdm_stream_t s) {
    if (!cfg_eps || !text_eps || !out || N <= 0 || n <= 1) return -1;
    PCDM_LAUNCH(rescale_cfg_kernel, dim3(N), dim3(1024), 0, (hipStream_t)s, cfg_eps, text_eps, out, n, guidance_rescale);
    PCDM_CHECK_LAUNCH();
    return 0;
}

// bf16 [rows, ldx] -> e4m3 [rows, ldy] (bytes), y = sat(x * scale); 8 elements per thread (16 B in, 8 B out); columns >= cols of a row
// (up to cols_pad) are written as zero: the K / V^T operands of pcdm_flash_attn_fp8
__global__ __launch_bounds__(256) void quantize_fp8_kernel(const u16* __restrict__ x, uint8_t* __restrict__ y, int64_t rows, int cols,
                                                           int cols_pad, int64_t ldx, int64_t ldy, float scale) {
    const int per_row = cols_pad / 8;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * per_row) return;
    const int64_t r = i / per_row;
    const int c = (int)(i - r * per_row) * 8;
    float v[8];
    if (c + 8 <= cols && (ldx & 7) == 0) {   // (rows start 16-byte aligned)
        const u16x8 a = *(const u16x8*)(x + r * ldx + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = bf2f(a[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = c + e < cols ? bf2f(x[r * ldx + c + e]) : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = fminf(fmaxf(v[e] * scale, -448.f), 448.f);
    u32x2 o = {pack4_fp8(v[0], v[1], v[2], v[3]), pack4_fp8(v[4], v[5], v[6], v[7])};
    *(u32x2*)(y + r * ldy + c) = o;
}

extern "C" int pcdm_quantize_fp8(const void* x, void* y, int64_t rows, int cols, int cols_pad, int64_t ldx, int64_t ldy, float scale,
                                 pcdm_stream_t s) {
    if (!x || !y || rows <= 0 || cols <= 0 || cols_pad < cols || cols_pad % 8 || ldy % 8 || ldy < cols_pad || ldx < cols) return -1;
    const int64_t total = rows * (cols_pad / 8);
    PCDM_LAUNCH(quantize_fp8_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, (const u16*)x, (uint8_t*)y, rows, cols, cols_pad,
                ldx, ldy, scale);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_softmax_rows(const float* s_in, void* p_out, int rows, int cols, int64_t ld_s, int64_t ld_p, float scale,
                                 pcdm_stream_t s) {
    if (!s_in || !p_out || rows <= 0 || cols <= 0 || cols > 8192) return -1;
    PCDM_LAUNCH(softmax_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)s, s_in, (u16*)p_out, cols, ld_s, ld_p,
                scale * 1.44269504088896341f);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_gaussian_sample(const float* moments, const float* noise, float* out, int B, int zc, int HW, float scale,
                                    pcdm_stream_t s) {
    if (!moments || !out || B <= 0 || zc <= 0 || HW <= 0) return -1;
    const int64_t total = (int64_t)B * zc * HW;
    PCDM_LAUNCH(gaussian_sample_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, moments, noise, out, zc, HW, scale,
                total);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_image_to_uint8(const float* x, void* out, int B, int cstride, int HW, pcdm_stream_t s) {
    if (!x || !out || B <= 0 || cstride < 3 || HW <= 0) return -1;
    const int64_t total = (int64_t)B * HW;
    PCDM_LAUNCH(image_to_uint8_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, x, (uint8_t*)out, cstride, HW, total);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_pixel_shuffle2(const void* in, void* out, int B, int H, int W, int C, pcdm_stream_t s) {
    if (!in || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7) || (((uintptr_t)in | (uintptr_t)out) & 15)) return -1;
    const int64_t total = (int64_t)B * 2 * H * 2 * W * (C / 8);
    PCDM_LAUNCH(pixel_shuffle2_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, (const u16*)in, (u16*)out, H, W, C / 8, total);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_advance_step(int32_t* step_dev, pcdm_stream_t s) {
    if (!step_dev) return -1;
    PCDM_LAUNCH(advance_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, step_dev);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t pcdm_metrics_ws_bytes(int N, int ref_n, int W, int H, float sigma) {
    if (N <= 0 || N > 65535 || (ref_n != 1 && ref_n != N) || W <= 0 || H <= 0) return -1;
    int64_t bytes = (int64_t)(N + ref_n) * kMetSlices * 2 * sizeof(float);   // (pcdm_psnr: N * kMetSlices doubles, never more than this)
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
    double* ws_part = (double*)((char*)ws + (size_t)(N + ref_n) * kMetSlices * 2 * sizeof(float));
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
    return (int64_t)(N + ref_n) * kMetSlices * 2 * sizeof(float) + (int64_t)N * tiles * sizeof(double);
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
    double* ws_part = (double*)((char*)ws + (size_t)(N + ref_n) * kMetSlices * 2 * sizeof(float));
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

// ---- LPIPS v0.1, net = 'alex' (the paper's second per-pair metric; the reference's metrics.py goes through the lpips package) in exact fp32 -------
// scaling layer -> AlexNet features (five convolutions with bias + ReLU, two 3x3 / stride-2 max-pools) -> per tap: channel-normalise both
// images, squared difference weighted by the 1x1 "lin" layer, spatial mean -> sum of the five taps.  Both images of every pair go through the
// network as ONE batch (candidates first, then the references: N + ref_n images), so each weight is read once per call.
// Activations are NHWC fp32.  The convolutions are implicit GEMMs on the fp32-input MFMA (pcdm_device.h: mfma_f32_16x16x4): M = batch Ho Wo,
// N = Cout, K = kh kw Cin -- a k-ordered fmaf chain per output, no reduced-precision operand anywhere (bf16 operands cost 5e-6 .. 9e-5 of the
// result, LPIPS differences between methods sit in the third decimal).  No atomics: per-workgroup fp64 partials of the spatial means, added in
// index order by one last launch, so reruns and batch permutations are bit-identical; an identical pair is exactly 0.
namespace {
constexpr int kLpSlices = 32;        // pixel slices per pair and tap of the distance pass
constexpr int kLpMaxC = 384;         // widest tap (six channels per lane)
constexpr int kLpChan[5] = {64, 192, 384, 256, 256};

struct LpSrc {             // window origin into uint8 NHWC [n, Hi, Wi, 3] or fp32 NCHW [n, 3, Hi, Wi]
    const void* p;
    int Hi, Wi, x0, y0;
};

// out fp32 NHWC [N + ref_n, H, W, 4] (channel 3 = 0: conv1's Cin padded to one 16-byte fragment) <- the scaling layer of the two windows:
// x = p / 255 for uint8, 2 x - 1 when normalize, then (x - shift[c]) / scale[c], every step in fp32 (not folded into conv1: other roundings)
__global__ __launch_bounds__(256) void lpips_input_kernel(LpSrc a, LpSrc b, int N, int f32, int normalize, int W, int H, int64_t total,
                                                          float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over (image, y, x)
    if (i >= total) return;
    const int x = (int)(i % W);
    const int64_t t = i / W;
    const int y = (int)(t % H), img = (int)(t / H);
    const LpSrc s = img < N ? a : b;
    const int n = img < N ? img : img - N;
    const int64_t plane = (int64_t)s.Hi * s.Wi, pix = (int64_t)(s.y0 + y) * s.Wi + s.x0 + x;
    const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = f32 ? ((const float*)s.p)[((int64_t)n * 3 + c) * plane + pix] : (float)((const uint8_t*)s.p)[((int64_t)n * plane + pix) * 3 + c] / 255.0f;
        if (normalize) v = 2.0f * v - 1.0f;
        o[c] = (v - shift[c]) / scale[c];
    }
    *(f32x4*)(out + i * 4) = o;
}

struct ConvF32 {
    const float* x;        // NHWC [B, Hi, Wi, Cin], Cin % 4 == 0
    const float* w;        // packed [Kpad / 4][Npad][4] (pcdm_pack_lpips_conv), k = (ky kw + kx) Cin + c
    const float* bias;     // [Npad]
    float* out;            // channel 0 of the output slice: pixel m, channel n at out[m * ldo + n] (ldo = Cout: a tight NHWC [B, Ho, Wo, Cout])
    int Hi, Wi, Cin, Ho, Wo, Cout, Npad, kh, kw, stride, pad_h, pad_w, Kpad, M, relu, ldo;
};

// One wave = a 32 x 64 output tile (2 x 4 accumulators of 16 x 16: eight independent MFMA chains), four waves along M per workgroup, operands
// straight from global memory / L2 (the whole LPIPS call is a few GFLOP; no LDS stage).  Per 16 k: lane (r, g) loads the 16 bytes
// k0 + 4g .. + 3 of its two rows' patches -- Cin % 4 == 0, so a fragment never straddles a tap and an out-of-image tap is one zero fragment,
// not a clamped read -- and of its four weight columns, then runs four MFMA steps per accumulator (mfma_f32_16x16x4_quad).
// The tap (ky, kx, c) of a lane advances by 16 channels per step without a division.  M and N tails: rows >= M load zeros and are not stored,
// 16-column sub-tiles beyond Npad and the second row block of a tile that ends in the first are skipped (wave-uniform).
__global__ __launch_bounds__(256) void conv_f32_kernel(ConvF32 p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int m0 = (blockIdx.x * 4 + wave) * 32, n0 = blockIdx.y * 64;
    if (m0 >= p.M) return;
    const int nsub = imin(4, (p.Npad - n0) / 16);
    const bool two = m0 + 16 < p.M;
    const float* xb[2];
    int iy0[2], ix0[2];
    bool valid[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int m = m0 + 16 * t + r;
        valid[t] = m < p.M;
        const int mm = valid[t] ? m : 0;
        const int b = mm / (p.Ho * p.Wo), q = mm - b * p.Ho * p.Wo;
        const int oy = q / p.Wo, ox = q - oy * p.Wo;
        iy0[t] = oy * p.stride - p.pad_h;
        ix0[t] = ox * p.stride - p.pad_w;
        xb[t] = p.x + (int64_t)b * p.Hi * p.Wi * p.Cin;
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    int c = 4 * g, kx = 0, ky = 0;
    while (c >= p.Cin) {
        c -= p.Cin;
        if (++kx == p.kw) { kx = 0; ++ky; }
    }
    const float* wp = p.w + ((int64_t)g * p.Npad + n0 + r) * 4;
    for (int k0 = 0; k0 < p.Kpad; k0 += 16) {
        f32x4 a[2], b[4];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int iy = iy0[t] + ky, ix = ix0[t] + kx;
            const bool ok = valid[t] && ky < p.kh && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
            a[t] = ok ? *(const f32x4*)(xb[t] + ((int64_t)iy * p.Wi + ix) * p.Cin + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = j < nsub ? *(const f32x4*)(wp + j * 64) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nsub) {
                acc[0][j] = mfma_f32_16x16x4_quad(a[0], b[j], acc[0][j]);
                if (two) acc[1][j] = mfma_f32_16x16x4_quad(a[1], b[j], acc[1][j]);
            }
        wp += (int64_t)16 * p.Npad;
        c += 16;
        while (c >= p.Cin) {
            c -= p.Cin;
            if (++kx == p.kw) { kx = 0; ++ky; }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + 16 * j + r;
        if (j >= nsub || n >= p.Cout) continue;
        const float bv = p.bias[n];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int m = m0 + 16 * t + 4 * g + e;
                if (m >= p.M) continue;
                float v = acc[t][j][e] + bv;
                if (p.relu) v = v > 0.f ? v : (v != v ? v : 0.f);
                p.out[(int64_t)m * p.ldo + n] = v;
            }
    }
}

// MaxPool2d(3, stride 2), no padding, floor: every window lies inside the image.  NHWC fp32, four channels per lane.
// Pixel i / C4 of the output lies at out + (i / C4) * ldo4 four-channel groups (ldo4 = C4: a tight tensor; else a channel slice of a wider one).
__global__ __launch_bounds__(256) void maxpool3s2_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int Hi, int Wi, int Ho, int Wo, int C4,
                                                             int ldo4, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over (b, oy, ox, c / 4)
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    int64_t t = i / C4;
    const int64_t pix = t;
    const int ox = (int)(t % Wo);
    t /= Wo;
    const int oy = (int)(t % Ho), b = (int)(t / Ho);
    const f32x4* src = (const f32x4*)x + (((int64_t)b * Hi + 2 * oy) * Wi + 2 * ox) * C4 + c4;
    f32x4 m = src[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const f32x4 v = src[((int64_t)dy * Wi + dx) * C4];
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = v[e] > m[e] || v[e] != v[e] ? v[e] : m[e];
        }
    ((f32x4*)out)[pix * ldo4 + c4] = m;
}

// One tap: part[n * kLpSlices + slice] = sum over the slice's pixels of sum_c lin[c] (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2, f0 = image n,
// f1 = image N + (ref_n == 1 ? 0 : n) of the NHWC features [N + ref_n, P, C].  A wave per pixel: channels across the lanes, fp32 inside the
// pixel (as the network), the pixels of a wave added in fp64 in pixel order.
__global__ __launch_bounds__(256) void lpips_dist_kernel(const float* __restrict__ f, int N, int ref_n, int P, int C, const float* __restrict__ lin,
                                                         double* __restrict__ part) {
    __shared__ double red[4];
    const int n = blockIdx.y, sl = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = (P + kLpSlices - 1) / kLpSlices;
    const int pa = sl * per, pb = imin(P, pa + per);
    const float* f0 = f + (int64_t)n * P * C;
    const float* f1 = f + (int64_t)(N + (ref_n == 1 ? 0 : n)) * P * C;
    double acc = 0.0;
    for (int px = pa + wave; px < pb; px += 4) {
        float v0[kLpMaxC / 64], v1[kLpMaxC / 64], s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int j = 0; j < kLpMaxC / 64; ++j) {
            const int c = lane + 64 * j;
            v0[j] = c < C ? f0[(int64_t)px * C + c] : 0.f;
            v1[j] = c < C ? f1[(int64_t)px * C + c] : 0.f;
            s0 += v0[j] * v0[j];
            s1 += v1[j] * v1[j];
        }
        const float d0 = sqrtf(wave_sum(s0)) + 1e-10f, d1 = sqrtf(wave_sum(s1)) + 1e-10f;
        float tsum = 0.f;
#pragma unroll
        for (int j = 0; j < kLpMaxC / 64; ++j) {
            const int c = lane + 64 * j;
            const float e = v0[j] / d0 - v1[j] / d1;
            if (c < C) tsum += lin[c] * (e * e);
        }
        acc += (double)wave_sum(tsum);
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(int64_t)n * kLpSlices + sl] = (red[0] + red[1]) + (red[2] + red[3]);
}

// layers[l * N + n] = float(sum of the slices in index order / pixels of tap l); out[n] = their fp32 sum in tap order (as the lpips package adds
// its five fp32 maps); then np.argmin: the first minimum wins and a NaN ranks as the minimum
struct LpCounts { double px[5]; };
__global__ __launch_bounds__(256) void lpips_final_kernel(const double* __restrict__ part, int N, LpCounts cnt, float* __restrict__ out,
                                                          float* __restrict__ layers, int32_t* __restrict__ argmin) {
    for (int n = threadIdx.x; n < N; n += 256) {
        float tot = 0.f;
        for (int l = 0; l < 5; ++l) {
            double s = 0.0;
            for (int i = 0; i < kLpSlices; ++i) s += part[((int64_t)l * N + n) * kLpSlices + i];
            const float d = (float)(s / cnt.px[l]);
            if (layers) layers[l * N + n] = d;
            tot += d;
        }
        out[n] = tot;
    }
    __syncthreads();
    if (threadIdx.x == 0 && argmin) {
        int best = 0;
        float vb = out[0];
        for (int i = 1; i < N && vb == vb; ++i) {
            const float v = out[i];
            if (v != v || v < vb) { best = i; vb = v; }
        }
        *argmin = best;
    }
}

struct LpGeom { int h[5], w[5], hp[2], wp[2]; };   // the five taps' sizes; the two pooled sizes
inline bool lpips_geom(int H, int W, LpGeom* g) {
    if (H < 31 || W < 31) return false;               // below 31 the second pool has no 3 x 3 window left
    g->h[0] = (H + 4 - 11) / 4 + 1;  g->w[0] = (W + 4 - 11) / 4 + 1;
    g->hp[0] = (g->h[0] - 3) / 2 + 1; g->wp[0] = (g->w[0] - 3) / 2 + 1;
    g->h[1] = g->hp[0];              g->w[1] = g->wp[0];
    g->hp[1] = (g->h[1] - 3) / 2 + 1; g->wp[1] = (g->w[1] - 3) / 2 + 1;
    for (int l = 2; l < 5; ++l) { g->h[l] = g->hp[1]; g->w[l] = g->wp[1]; }
    return true;
}
inline int64_t lp_align(int64_t bytes) { return (bytes + 255) / 256 * 256; }
// workspace: [input B H W 4 | tap 1..5 | pool 1, 2 | partials 5 N kLpSlices fp64], each a multiple of 256 bytes; offsets in bytes
struct LpLayout { int64_t in, tap[5], pool[2], part, total; };
inline LpLayout lpips_layout(int N, int ref_n, int H, int W, const LpGeom& g) {
    const int64_t B = N + ref_n;
    LpLayout o;
    int64_t at = 0;
    o.in = at;  at += lp_align(B * H * W * 4 * (int64_t)sizeof(float));
    for (int l = 0; l < 5; ++l) { o.tap[l] = at; at += lp_align(B * g.h[l] * g.w[l] * kLpChan[l] * (int64_t)sizeof(float)); }
    for (int i = 0; i < 2; ++i) { o.pool[i] = at; at += lp_align(B * g.hp[i] * g.wp[i] * kLpChan[i] * (int64_t)sizeof(float)); }
    o.part = at; at += lp_align((int64_t)5 * N * kLpSlices * (int64_t)sizeof(double));
    o.total = at;
    return o;
}
inline bool lpips_sizes_ok(int N, int ref_n, int H, int W) {
    return N > 0 && N <= 65535 && (ref_n == 1 || ref_n == N) && H > 0 && W > 0 && (int64_t)(N + ref_n) * H * W < (int64_t)1 << 28;
}

// The output is the channel slice [off, off + Cout) of an NHWC tensor with ldo channels per pixel (ldo = Cout, off = 0: a tight tensor).
inline int conv_f32_launch(const float* x, int B, int Hi, int Wi, int Cin, const float* w, const float* bias, int Cout, int kh, int kw, int stride,
                           int pad_h, int pad_w, int relu, float* out, int ldo, int off, hipStream_t s) {
    if (!x || !w || !bias || !out || B <= 0 || Hi <= 0 || Wi <= 0 || Cin <= 0 || Cin % 4 || Cout <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || pad_h < 0 ||
        pad_w < 0 || off < 0 || ldo < Cout || off > ldo - Cout)
        return -1;
    if (((uintptr_t)x | (uintptr_t)w) & 15) return -1;
    if (Hi + 2 * (int64_t)pad_h < kh || Wi + 2 * (int64_t)pad_w < kw || pad_h >= 1 << 20 || pad_w >= 1 << 20) return -1;
    const int Ho = (Hi + 2 * pad_h - kh) / stride + 1, Wo = (Wi + 2 * pad_w - kw) / stride + 1;
    const int64_t M = (int64_t)B * Ho * Wo, K = (int64_t)kh * kw * Cin;
    const int Npad = (Cout + 15) / 16 * 16;
    if (M * ldo >= (int64_t)1 << 31 || (int64_t)B * Hi * Wi * Cin >= (int64_t)1 << 31 || K >= 1 << 24 || (Npad + 63) / 64 > 65535) return -1;
    ConvF32 p{x, w, bias, out + off, Hi, Wi, Cin, Ho, Wo, Cout, Npad, kh, kw, stride, pad_h, pad_w, (int)((K + 15) / 16 * 16), (int)M, relu, ldo};
    PCDM_LAUNCH(conv_f32_kernel, dim3((unsigned)((M + 127) / 128), (Npad + 63) / 64), dim3(256), 0, s, p);
    PCDM_CHECK_LAUNCH();
    return 0;
}
inline int maxpool_f32_launch(const float* x, int B, int Hi, int Wi, int C, float* out, int ldo, int off, hipStream_t s) {
    if (!x || !out || B <= 0 || Hi < 3 || Wi < 3 || C <= 0 || C % 4 || (((uintptr_t)x | (uintptr_t)out) & 15)) return -1;
    if (off < 0 || off % 4 || ldo % 4 || ldo < C || off > ldo - C) return -1;
    const int Ho = (Hi - 3) / 2 + 1, Wo = (Wi - 3) / 2 + 1;
    if ((int64_t)B * Hi * Wi * C >= (int64_t)1 << 31 || (int64_t)B * Ho * Wo * ldo >= (int64_t)1 << 31) return -1;
    const int64_t total = (int64_t)B * Ho * Wo * (C / 4);
    PCDM_LAUNCH(maxpool3s2_f32_kernel, grid1d(total, 256), dim3(256), 0, s, x, out + off, Hi, Wi, Ho, Wo, C / 4, ldo / 4, total);
    PCDM_CHECK_LAUNCH();
    return 0;
}
}  // namespace

extern "C" int pcdm_pack_lpips_conv(const float* w, const float* bias, int Cout, int Cin, int kh, int kw, float* out_w, float* out_bias, int* K_out,
                                    int* cin_out) {
    if (Cout <= 0 || Cin <= 0 || kh <= 0 || kw <= 0) return -1;
    const int Cp = (Cin + 3) / 4 * 4, Npad = (Cout + 15) / 16 * 16;
    const int64_t K = (int64_t)kh * kw * Cp, Kpad = (K + 15) / 16 * 16;
    if (K >= 1 << 24) return -1;
    if (K_out) *K_out = (int)Kpad;
    if (cin_out) *cin_out = Cp;
    if (out_w) {
        if (!w) return -1;
        for (int64_t i = 0; i < Kpad * Npad; ++i) out_w[i] = 0.f;
        for (int64_t n = 0; n < Cout; ++n)
            for (int c = 0; c < Cin; ++c)
                for (int t = 0; t < kh * kw; ++t) {
                    const int64_t k = (int64_t)t * Cp + c;
                    out_w[((k / 4) * Npad + n) * 4 + (k & 3)] = w[(n * Cin + c) * kh * kw + t];
                }
    }
    if (out_bias)
        for (int n = 0; n < Npad; ++n) out_bias[n] = (bias && n < Cout) ? bias[n] : 0.f;
    return Npad;
}

extern "C" int pcdm_conv2d_f32(const float* x, int B, int Hi, int Wi, int Cin, const float* w_packed, const float* bias, int Cout, int kh, int kw,
                               int stride, int pad, int relu, float* out, pcdm_stream_t s) {
    return conv_f32_launch(x, B, Hi, Wi, Cin, w_packed, bias, Cout, kh, kw, stride, pad, pad, relu, out, Cout, 0, (hipStream_t)s);
}

extern "C" int pcdm_maxpool3s2_f32(const float* x, int B, int Hi, int Wi, int C, float* out, pcdm_stream_t s) {
    return maxpool_f32_launch(x, B, Hi, Wi, C, out, C, 0, (hipStream_t)s);
}

extern "C" int64_t pcdm_lpips_ws_bytes(int N, int ref_n, int H, int W) {
    LpGeom g;
    if (!lpips_sizes_ok(N, ref_n, H, W) || !lpips_geom(H, W, &g)) return -1;
    return lpips_layout(N, ref_n, H, W, g).total;
}

extern "C" int pcdm_lpips(const void* img0, int N, int H0, int W0, const int32_t* win0, const void* img1, int ref_n, int H1, int W1,
                          const int32_t* win1, int is_f32, int normalize, const pcdm_lpips_weights* wts, float* out, float* layers, int32_t* argmin,
                          void* ws, int64_t ws_bytes, pcdm_stream_t s) {
    if (!img0 || !img1 || !wts || !out || !ws || ((uintptr_t)ws & 15)) return -1;
    if (!met_window_ok(H0, W0, win0) || !met_window_ok(H1, W1, win1) || win0[2] != win1[2] || win0[3] != win1[3]) return -1;
    const int W = win0[2], H = win0[3], B = N + ref_n;
    LpGeom g;
    if (!lpips_sizes_ok(N, ref_n, H, W) || !lpips_geom(H, W, &g)) return -1;
    if ((int64_t)N * H0 * W0 * 3 >= (int64_t)1 << 31 || (int64_t)ref_n * H1 * W1 * 3 >= (int64_t)1 << 31) return -1;
    for (int l = 0; l < 5; ++l)
        if (!wts->conv_w[l] || !wts->conv_b[l] || !wts->lin[l]) return -1;
    const LpLayout lay = lpips_layout(N, ref_n, H, W, g);
    if (ws_bytes < lay.total) return -1;
    char* base = (char*)ws;
    float* x = (float*)(base + lay.in);
    float* tap[5];
    for (int l = 0; l < 5; ++l) tap[l] = (float*)(base + lay.tap[l]);
    float* pool[2] = {(float*)(base + lay.pool[0]), (float*)(base + lay.pool[1])};
    double* part = (double*)(base + lay.part);
    hipStream_t st = (hipStream_t)s;
    const int64_t total = (int64_t)B * H * W;
    PCDM_LAUNCH(lpips_input_kernel, grid1d(total, 256), dim3(256), 0, st, LpSrc{img0, H0, W0, win0[0], win0[1]}, LpSrc{img1, H1, W1, win1[0], win1[1]}, N,
                is_f32, normalize, W, H, total, x);
    PCDM_CHECK_LAUNCH();
    int rc = conv_f32_launch(x, B, H, W, 4, wts->conv_w[0], wts->conv_b[0], 64, 11, 11, 4, 2, 2, 1, tap[0], 64, 0, st);
    if (rc == 0) rc = maxpool_f32_launch(tap[0], B, g.h[0], g.w[0], 64, pool[0], 64, 0, st);
    if (rc == 0) rc = conv_f32_launch(pool[0], B, g.hp[0], g.wp[0], 64, wts->conv_w[1], wts->conv_b[1], 192, 5, 5, 1, 2, 2, 1, tap[1], 192, 0, st);
    if (rc == 0) rc = maxpool_f32_launch(tap[1], B, g.h[1], g.w[1], 192, pool[1], 192, 0, st);
    if (rc == 0) rc = conv_f32_launch(pool[1], B, g.hp[1], g.wp[1], 192, wts->conv_w[2], wts->conv_b[2], 384, 3, 3, 1, 1, 1, 1, tap[2], 384, 0, st);
    if (rc == 0) rc = conv_f32_launch(tap[2], B, g.h[2], g.w[2], 384, wts->conv_w[3], wts->conv_b[3], 256, 3, 3, 1, 1, 1, 1, tap[3], 256, 0, st);
    if (rc == 0) rc = conv_f32_launch(tap[3], B, g.h[3], g.w[3], 256, wts->conv_w[4], wts->conv_b[4], 256, 3, 3, 1, 1, 1, 1, tap[4], 256, 0, st);
    if (rc != 0) return rc;
    LpCounts cnt;
    for (int l = 0; l < 5; ++l) {
        cnt.px[l] = (double)g.h[l] * (double)g.w[l];
        PCDM_LAUNCH(lpips_dist_kernel, dim3(kLpSlices, N), dim3(256), 0, st, tap[l], N, ref_n, g.h[l] * g.w[l], kLpChan[l], wts->lin[l],
                    part + (int64_t)l * N * kLpSlices);
        PCDM_CHECK_LAUNCH();
    }
    PCDM_LAUNCH(lpips_final_kernel, dim3(1), dim3(256), 0, st, part, N, cnt, out, layers, argmin);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_conv2d_f32_ex(const float* x, int B, int Hi, int Wi, int Cin, const float* w_packed, const float* bias, int Cout, int kh, int kw,
                                  int stride, int pad_h, int pad_w, int relu, float* out, int out_pitch, int out_offset, pcdm_stream_t s) {
    return conv_f32_launch(x, B, Hi, Wi, Cin, w_packed, bias, Cout, kh, kw, stride, pad_h, pad_w, relu, out, out_pitch, out_offset, (hipStream_t)s);
}

extern "C" int pcdm_maxpool3s2_f32_ex(const float* x, int B, int Hi, int Wi, int C, float* out, int out_pitch, int out_offset, pcdm_stream_t s) {
    return maxpool_f32_launch(x, B, Hi, Wi, C, out, out_pitch, out_offset, (hipStream_t)s);
}

// ---- FID (the paper's third metric; the reference's metrics.py:23-257 + inception.py): torchvision's InceptionV3 trunk in exact fp32 -----------------
// input stage (bilinear 299 x 299 resample + the reference's remap) -> 94 x [convolution, BatchNorm folded on the host, ReLU] on conv_f32_kernel,
// every branch writing its channel slice of the block's concatenated tensor -> global average pool -> fp64 sum / Gram accumulation over the
// samples -> mean and covariance.  Like LPIPS: NHWC fp32 activations, no atomics, fixed summation orders, no allocation, no host synchronisation.
namespace {
// out fp32 NHWC [N, Ho, Wo, 4] (channel 3 = 0) <- the window (x0, y0, Ws, Hs) of uint8 NHWC [N, Hi, Wi, 3] (x = p / 255) or fp32 NCHW [N, 3, Hi, Wi].
// resize: bilinear, align_corners = False, no antialias (F.interpolate): source coordinate (o + 0.5) Ws / Wo - 0.5 clamped at 0, as the exact
// rational ((2 o + 1) Ws - Wo) / (2 Wo); the neighbour index is clamped at the window's last pixel.  normalize: the reference's remap
// x s_c / 0.5 + (m_c - 0.5) / 0.5.  Everything in fp64, rounded to fp32 once.
__global__ __launch_bounds__(256) void inception_input_kernel(LpSrc s, int Hs, int Ws, int f32, int resize, int normalize, int Ho, int Wo, int64_t total,
                                                              float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over (image, y, x)
    if (i >= total) return;
    const int x = (int)(i % Wo);
    const int64_t t = i / Wo;
    const int y = (int)(t % Ho), n = (int)(t / Ho);
    int xa = x, xb = x, ya = y, yb = y;
    double lx = 0.0, ly = 0.0;
    if (resize) {
        const int64_t nx = (int64_t)(2 * x + 1) * Ws - Wo, ny = (int64_t)(2 * y + 1) * Hs - Ho;
        if (nx > 0) { xa = (int)(nx / (2 * Wo)); lx = (double)(nx % (2 * Wo)) / (double)(2 * Wo); } else xa = 0;
        if (ny > 0) { ya = (int)(ny / (2 * Ho)); ly = (double)(ny % (2 * Ho)) / (double)(2 * Ho); } else ya = 0;
        xa = imin(xa, Ws - 1);
        ya = imin(ya, Hs - 1);
        xb = imin(xa + 1, Ws - 1);
        yb = imin(ya + 1, Hs - 1);
    }
    const int64_t plane = (int64_t)s.Hi * s.Wi;
    const int64_t p00 = (int64_t)(s.y0 + ya) * s.Wi + s.x0 + xa, p01 = (int64_t)(s.y0 + ya) * s.Wi + s.x0 + xb;
    const int64_t p10 = (int64_t)(s.y0 + yb) * s.Wi + s.x0 + xa, p11 = (int64_t)(s.y0 + yb) * s.Wi + s.x0 + xb;
    const double sc[3] = {0.229 / 0.5, 0.224 / 0.5, 0.225 / 0.5}, sh[3] = {(0.485 - 0.5) / 0.5, (0.456 - 0.5) / 0.5, (0.406 - 0.5) / 0.5};
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double v00, v01, v10, v11;
        if (f32) {
            const float* q = (const float*)s.p + ((int64_t)n * 3 + c) * plane;
            v00 = q[p00]; v01 = q[p01]; v10 = q[p10]; v11 = q[p11];
        } else {
            const uint8_t* q = (const uint8_t*)s.p + (int64_t)n * plane * 3 + c;
            v00 = q[p00 * 3] / 255.0; v01 = q[p01 * 3] / 255.0; v10 = q[p10 * 3] / 255.0; v11 = q[p11 * 3] / 255.0;
        }
        double v = (1.0 - ly) * ((1.0 - lx) * v00 + lx * v01) + ly * ((1.0 - lx) * v10 + lx * v11);
        if (normalize) v = v * sc[c] + sh[c];
        o[c] = (float)v;
    }
    *(f32x4*)(out + i * 4) = o;
}

// F.avg_pool2d(x, 3, 1, 1), count_include_pad: the nine taps in (dy, dx) order in fp32, zeros outside, divided by 9.  NHWC, four channels per lane.
__global__ __launch_bounds__(256) void avgpool3_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W, int C4, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over (b, y, x, c / 4)
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    int64_t t = i / C4;
    const int px = (int)(t % W);
    t /= W;
    const int py = (int)(t % H), b = (int)(t / H);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int yy = py + dy, xx = px + dx;
            if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
            const f32x4 v = ((const f32x4*)x)[(((int64_t)b * H + yy) * W + xx) * C4 + c4];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += v[e];
        }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] /= 9.0f;
    ((f32x4*)out)[i] = acc;
}

// out[b, c] = float(sum over the P pixels, in pixel order, in fp64 / P) of NHWC [B, P, C]: one lane per output, lanes along c
__global__ __launch_bounds__(256) void global_avgpool_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int P, int C, int total) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = i % C, b = i / C;
    const float* src = x + (int64_t)b * P * C + c;
    double acc = 0.0;
    for (int p = 0; p < P; ++p) acc += (double)src[(int64_t)p * C];
    out[i] = (float)(acc / (double)P);
}

// One lane per output: gram[i, j] += sum_b x[b, i] x[b, j] (i * D + j < D D), sum[j] += sum_b x[b, j] (the D lanes after those), the samples in
// order, in fp64 (the product of two fp32 values is exact there).  Adding a batch continues the chain the previous one left, so the state after
// n samples does not depend on how they were split into batches.
__global__ __launch_bounds__(256) void fid_accumulate_kernel(const float* __restrict__ x, int B, int D, double* __restrict__ sum, double* __restrict__ gram) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, DD = (int64_t)D * D;
    if (t >= DD + D) return;
    if (t < DD) {
        const int i = (int)(t / D), j = (int)(t % D);
        double acc = gram[t];
        for (int b = 0; b < B; ++b) acc += (double)x[(int64_t)b * D + i] * (double)x[(int64_t)b * D + j];
        gram[t] = acc;
    } else {
        const int j = (int)(t - DD);
        double acc = sum[j];
        for (int b = 0; b < B; ++b) acc += (double)x[(int64_t)b * D + j];
        sum[j] = acc;
    }
}

// mu = sum / n; sigma[i, j] = (gram[i, j] - sum[i] sum[j] / n) / (n - 1): np.cov(rowvar=False) (ddof 1), symmetric bit for bit
__global__ __launch_bounds__(256) void fid_finalize_kernel(const double* __restrict__ sum, const double* __restrict__ gram, double n, int D,
                                                           double* __restrict__ mu, double* __restrict__ sigma) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, DD = (int64_t)D * D;
    if (t >= DD + D) return;
    if (t < DD) {
        const int i = (int)(t / D), j = (int)(t % D);
        sigma[t] = (gram[t] - sum[i] * sum[j] / n) / (n - 1.0);
    } else {
        mu[t - DD] = sum[t - DD] / n;
    }
}

inline int avgpool3_f32_launch(const float* x, int B, int H, int W, int C, float* out, hipStream_t s) {
    if (!x || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 || (((uintptr_t)x | (uintptr_t)out) & 15)) return -1;
    if ((int64_t)B * H * W * C >= (int64_t)1 << 31) return -1;
    const int64_t total = (int64_t)B * H * W * (C / 4);
    PCDM_LAUNCH(avgpool3_f32_kernel, grid1d(total, 256), dim3(256), 0, s, x, out, H, W, C / 4, total);
    PCDM_CHECK_LAUNCH();
    return 0;
}
inline int global_avgpool_f32_launch(const float* x, int B, int P, int C, float* out, hipStream_t s) {
    if (!x || !out || B <= 0 || P <= 0 || C <= 0 || (int64_t)B * P * C >= (int64_t)1 << 31) return -1;
    PCDM_LAUNCH(global_avgpool_f32_kernel, grid1d((int64_t)B * C, 256), dim3(256), 0, s, x, out, P, C, B * C);
    PCDM_CHECK_LAUNCH();
    return 0;
}
inline int inception_input_launch(const void* img, int N, int Hi, int Wi, const int32_t* win, int is_f32, int resize, int normalize, float* out,
                                  hipStream_t s) {
    if (!img || !out || N <= 0 || !met_window_ok(Hi, Wi, win) || ((uintptr_t)out & 15)) return -1;
    const int Ho = resize ? 299 : win[3], Wo = resize ? 299 : win[2];
    if ((int64_t)N * Hi * Wi * 3 >= (int64_t)1 << 31 || (int64_t)N * Ho * Wo * 4 >= (int64_t)1 << 31) return -1;
    const int64_t total = (int64_t)N * Ho * Wo;
    PCDM_LAUNCH(inception_input_kernel, grid1d(total, 256), dim3(256), 0, s, LpSrc{img, Hi, Wi, win[0], win[1]}, win[3], win[2], is_f32, resize, normalize,
                Ho, Wo, total, out);
    PCDM_CHECK_LAUNCH();
    return 0;
}

// ---- the trunk as a table.  Buffers: X = the input stage's output, A / B = a block's input and output (they swap), T / U = a branch's intermediates,
// P = the 3 x 3 average of the block input.  The convolutions are numbered in the order they are appended = include/pcdm.h's order.
enum { kIncX = 0, kIncA, kIncB, kIncT, kIncU, kIncP, kIncBufs };
enum { kIncConv = 0, kIncMax, kIncAvg };
constexpr int kIncConvs = 94, kIncMaxOps = 128;
struct IncOp { int kind, src, dst, Hi, Wi, Cin, Cout, kh, kw, stride, ph, pw, ldo, off, conv; };
struct IncPlan {
    IncOp op[kIncMaxOps];
    int n = 0, convs = 0, H = 0, W = 0, C = 0, buf = kIncX;   // the running tensor
    int64_t elems[kIncBufs] = {0, 0, 0, 0, 0, 0};             // per image
    bool ok = true;
    void use(int buf_, int64_t e) { if (e > elems[buf_]) elems[buf_] = e; }
    // a convolution src [Hi, Wi, Cin] -> channels [off, off + Cout) of dst [Ho, Wo, ldo]; returns through ho / wo
    void conv(int src, int Hi, int Wi, int Cin, int dst, int Cout, int kh, int kw, int stride, int ph, int pw, int ldo, int off, int* ho, int* wo) {
        if (Hi + 2 * ph < kh || Wi + 2 * pw < kw || n >= kIncMaxOps) { ok = false; *ho = *wo = 1; return; }
        *ho = (Hi + 2 * ph - kh) / stride + 1;
        *wo = (Wi + 2 * pw - kw) / stride + 1;
        op[n++] = IncOp{kIncConv, src, dst, Hi, Wi, Cin, Cout, kh, kw, stride, ph, pw, ldo, off, convs++};
        use(dst, (int64_t)*ho * *wo * ldo);
    }
    void pool(int kind, int src, int Hi, int Wi, int Cc, int dst, int ldo, int off, int* ho, int* wo) {
        if ((kind == kIncMax && (Hi < 3 || Wi < 3)) || n >= kIncMaxOps) { ok = false; *ho = *wo = 1; return; }
        *ho = kind == kIncMax ? (Hi - 3) / 2 + 1 : Hi;
        *wo = kind == kIncMax ? (Wi - 3) / 2 + 1 : Wi;
        op[n++] = IncOp{kind, src, dst, Hi, Wi, Cc, Cc, 3, 3, kind == kIncMax ? 2 : 1, 0, 0, ldo, off, -1};
        use(dst, (int64_t)*ho * *wo * ldo);
    }
    // same-size helpers on the running tensor (stride 1, "same" padding): the branches of a Mixed block
    void same(int src, int Cin, int dst, int Cout, int kh, int kw, int ldo, int off) {
        int ho, wo;
        conv(src, H, W, Cin, dst, Cout, kh, kw, 1, kh / 2, kw / 2, ldo, off, &ho, &wo);
    }
    int other() const { return buf == kIncA ? kIncB : kIncA; }
    void done(int Cout, int ho, int wo) { buf = other(); C = Cout; H = ho; W = wo; }
    void stem(int Cout, int k, int stride, int pad) {
        int ho, wo;
        conv(buf, H, W, C, other(), Cout, k, k, stride, pad, pad, Cout, 0, &ho, &wo);
        done(Cout, ho, wo);
    }
    void stem_pool() {
        int ho, wo;
        pool(kIncMax, buf, H, W, C, other(), C, 0, &ho, &wo);
        done(C, ho, wo);
    }
    void inception_a(int pf) {
        const int in = buf, out = other(), ldo = 224 + pf;
        same(in, C, out, 64, 1, 1, ldo, 0);
        same(in, C, kIncT, 48, 1, 1, 48, 0);
        same(kIncT, 48, out, 64, 5, 5, ldo, 64);
        same(in, C, kIncT, 64, 1, 1, 64, 0);
        same(kIncT, 64, kIncU, 96, 3, 3, 96, 0);
        same(kIncU, 96, out, 96, 3, 3, ldo, 128);
        int ho, wo;
        pool(kIncAvg, in, H, W, C, kIncP, C, 0, &ho, &wo);
        same(kIncP, C, out, pf, 1, 1, ldo, 224);
        done(ldo, H, W);
    }
    void inception_b() {
        const int in = buf, out = other(), ldo = 384 + 96 + C;
        int ho, wo, h2, w2;
        conv(in, H, W, C, out, 384, 3, 3, 2, 0, 0, ldo, 0, &ho, &wo);
        same(in, C, kIncT, 64, 1, 1, 64, 0);
        same(kIncT, 64, kIncU, 96, 3, 3, 96, 0);
        conv(kIncU, H, W, 96, out, 96, 3, 3, 2, 0, 0, ldo, 384, &h2, &w2);
        pool(kIncMax, in, H, W, C, out, ldo, 480, &h2, &w2);
        done(ldo, ho, wo);
    }
    void inception_c(int c7) {
        const int in = buf, out = other(), ldo = 768;
        same(in, C, out, 192, 1, 1, ldo, 0);
        same(in, C, kIncT, c7, 1, 1, c7, 0);
        same(kIncT, c7, kIncU, c7, 1, 7, c7, 0);
        same(kIncU, c7, out, 192, 7, 1, ldo, 192);
        same(in, C, kIncT, c7, 1, 1, c7, 0);
        same(kIncT, c7, kIncU, c7, 7, 1, c7, 0);
        same(kIncU, c7, kIncT, c7, 1, 7, c7, 0);
        same(kIncT, c7, kIncU, c7, 7, 1, c7, 0);
        same(kIncU, c7, out, 192, 1, 7, ldo, 384);
        int ho, wo;
        pool(kIncAvg, in, H, W, C, kIncP, C, 0, &ho, &wo);
        same(kIncP, C, out, 192, 1, 1, ldo, 576);
        done(ldo, H, W);
    }
    void inception_d() {
        const int in = buf, out = other(), ldo = 320 + 192 + C;
        int ho, wo, h2, w2;
        same(in, C, kIncT, 192, 1, 1, 192, 0);
        conv(kIncT, H, W, 192, out, 320, 3, 3, 2, 0, 0, ldo, 0, &ho, &wo);
        same(in, C, kIncT, 192, 1, 1, 192, 0);
        same(kIncT, 192, kIncU, 192, 1, 7, 192, 0);
        same(kIncU, 192, kIncT, 192, 7, 1, 192, 0);
        conv(kIncT, H, W, 192, out, 192, 3, 3, 2, 0, 0, ldo, 320, &h2, &w2);
        pool(kIncMax, in, H, W, C, out, ldo, 512, &h2, &w2);
        done(ldo, ho, wo);
    }
    void inception_e() {
        const int in = buf, out = other(), ldo = 2048;
        same(in, C, out, 320, 1, 1, ldo, 0);
        same(in, C, kIncT, 384, 1, 1, 384, 0);
        same(kIncT, 384, out, 384, 1, 3, ldo, 320);
        same(kIncT, 384, out, 384, 3, 1, ldo, 704);
        same(in, C, kIncT, 448, 1, 1, 448, 0);
        same(kIncT, 448, kIncU, 384, 3, 3, 384, 0);
        same(kIncU, 384, out, 384, 1, 3, ldo, 1088);
        same(kIncU, 384, out, 384, 3, 1, ldo, 1472);
        int ho, wo;
        pool(kIncAvg, in, H, W, C, kIncP, C, 0, &ho, &wo);
        same(kIncP, C, out, 192, 1, 1, ldo, 1856);
        done(ldo, H, W);
    }
};

// the trunk up to the block whose output has `dims` channels, on an H x W network input; false: dims or a size the trunk cannot take
inline bool inception_plan(int H, int W, int dims, IncPlan* p) {
    if (dims != 64 && dims != 192 && dims != 768 && dims != 2048) return false;
    if (H < 3 || W < 3 || H > 4096 || W > 4096) return false;
    p->H = H; p->W = W; p->C = 4; p->buf = kIncX;
    p->use(kIncX, (int64_t)H * W * 4);
    p->stem(32, 3, 2, 0);                      // Conv2d_1a_3x3   (X -> A; from here A <-> B)
    p->stem(32, 3, 1, 0);                      // Conv2d_2a_3x3
    p->stem(64, 3, 1, 1);                      // Conv2d_2b_3x3
    p->stem_pool();
    if (dims > 64) {
        p->stem(80, 1, 1, 0);                  // Conv2d_3b_1x1
        p->stem(192, 3, 1, 0);                 // Conv2d_4a_3x3
        p->stem_pool();
    }
    if (dims > 192) {
        p->inception_a(32);                    // Mixed_5b, 5c, 5d
        p->inception_a(64);
        p->inception_a(64);
        p->inception_b();                      // Mixed_6a
        p->inception_c(128);                   // Mixed_6b .. 6e
        p->inception_c(160);
        p->inception_c(160);
        p->inception_c(192);
    }
    if (dims > 768) {
        p->inception_d();                      // Mixed_7a
        p->inception_e();                      // Mixed_7b, 7c
        p->inception_e();
    }
    return p->ok && p->C == dims;
}
inline bool inception_sizes_ok(int B, int H, int W) { return B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)B * H * W < (int64_t)1 << 27; }
// workspace: the six buffers in enum order, each a multiple of 256 bytes; offsets in bytes
struct IncLayout { int64_t at[kIncBufs], total; };
inline IncLayout inception_layout(int B, const IncPlan& p) {
    IncLayout o;
    int64_t at = 0;
    for (int i = 0; i < kIncBufs; ++i) { o.at[i] = at; at += lp_align((int64_t)B * p.elems[i] * (int64_t)sizeof(float)); }
    o.total = at;
    return o;
}
}  // namespace

extern "C" int pcdm_avgpool3_f32(const float* x, int B, int H, int W, int C, float* out, pcdm_stream_t s) {
    return avgpool3_f32_launch(x, B, H, W, C, out, (hipStream_t)s);
}

extern "C" int pcdm_global_avgpool_f32(const float* x, int B, int P, int C, float* out, pcdm_stream_t s) {
    return global_avgpool_f32_launch(x, B, P, C, out, (hipStream_t)s);
}

extern "C" int pcdm_inception_input(const void* img, int N, int Hi, int Wi, const int32_t* win, int is_f32, int resize, int normalize, float* out,
                                    pcdm_stream_t s) {
    return inception_input_launch(img, N, Hi, Wi, win, is_f32, resize, normalize, out, (hipStream_t)s);
}

extern "C" int64_t pcdm_inception_ws_bytes(int B, int H, int W, int dims) {
    IncPlan p;
    if (!inception_sizes_ok(B, H, W) || !inception_plan(H, W, dims, &p)) return -1;
    return inception_layout(B, p).total;
}

extern "C" int pcdm_inception_features(const void* img, int N, int Hi, int Wi, const int32_t* win, int is_f32, int resize, int normalize, int dims,
                                       const pcdm_inception_weights* wts, float* out, void* ws, int64_t ws_bytes, pcdm_stream_t s) {
    if (!img || !wts || !out || !ws || ((uintptr_t)ws & 15) || !met_window_ok(Hi, Wi, win)) return -1;
    const int H = resize ? 299 : win[3], W = resize ? 299 : win[2];
    IncPlan p;
    if (!inception_sizes_ok(N, H, W) || !inception_plan(H, W, dims, &p)) return -1;
    for (int i = 0; i < p.convs; ++i)
        if (!wts->w[i] || !wts->bias[i]) return -1;
    const IncLayout lay = inception_layout(N, p);
    if (ws_bytes < lay.total) return -1;
    float* buf[kIncBufs];
    for (int i = 0; i < kIncBufs; ++i) buf[i] = (float*)((char*)ws + lay.at[i]);
    hipStream_t st = (hipStream_t)s;
    int rc = inception_input_launch(img, N, Hi, Wi, win, is_f32, resize, normalize, buf[kIncX], st);
    for (int i = 0; i < p.n && rc == 0; ++i) {
        const IncOp& o = p.op[i];
        if (o.kind == kIncConv)
            rc = conv_f32_launch(buf[o.src], N, o.Hi, o.Wi, o.Cin, wts->w[o.conv], wts->bias[o.conv], o.Cout, o.kh, o.kw, o.stride, o.ph, o.pw, 1, buf[o.dst],
                                 o.ldo, o.off, st);
        else if (o.kind == kIncMax)
            rc = maxpool_f32_launch(buf[o.src], N, o.Hi, o.Wi, o.Cin, buf[o.dst], o.ldo, o.off, st);
        else
            rc = avgpool3_f32_launch(buf[o.src], N, o.Hi, o.Wi, o.Cin, buf[o.dst], st);
    }
    if (rc == 0) rc = global_avgpool_f32_launch(buf[p.buf], N, p.H * p.W, p.C, out, st);
    return rc;
}

extern "C" int pcdm_fid_accumulate(const float* feat, int B, int D, double* sum, double* gram, pcdm_stream_t s) {
    if (!feat || !sum || !gram || B <= 0 || D <= 0 || D > 8192 || (int64_t)B * D >= (int64_t)1 << 31) return -1;
    PCDM_LAUNCH(fid_accumulate_kernel, grid1d((int64_t)D * D + D, 256), dim3(256), 0, (hipStream_t)s, feat, B, D, sum, gram);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_fid_finalize(const double* sum, const double* gram, int64_t n, int D, double* mu, double* sigma, pcdm_stream_t s) {
    if (!sum || !gram || !mu || !sigma || n < 2 || D <= 0 || D > 8192) return -1;
    PCDM_LAUNCH(fid_finalize_kernel, grid1d((int64_t)D * D + D, 256), dim3(256), 0, (hipStream_t)s, sum, gram, (double)n, D, mu, sigma);
    PCDM_CHECK_LAUNCH();
    return 0;
}
