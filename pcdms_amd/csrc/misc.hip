// Small / elementwise kernels of the stage-2 denoise step (SURVEY.md §2.1 K12, K13 and the
// input assembly of stage2_inpaint_pipeline.py:499-501).  All HBM- or latency-bound; 16-byte
// vector accesses where the layout allows, device-resident step index so one captured hipGraph
// replays for every timestep.
#include "pcdm_device.h"
#include "../../include/pcdm.h"
#include "image_common.h"

namespace {
// the device step counter bounded into a table of `rows` rows (NULL counter: row 0), as pcdm_gemm_detail::bounded_step: a value outside
// [0, rows) reads the nearest valid row instead of foreign memory and raises *err (every lane stores the same 1: a benign race)
__device__ __forceinline__ int table_row(const int32_t* step_dev, int rows, int32_t* err) {
    int st = step_dev ? *step_dev : 0;
    if (st < 0 || st >= rows) {
        if (err) *err = 1;
        st = st < 0 ? 0 : rows - 1;
    }
    return st;
}

// out[b, j]: diffusers Timesteps (flip_sin_to_cos => [cos | sin]).  T = int64_t (the integer schedules) or float (the fractional timesteps of
// the sigma-space samplers): the timestep is converted to fp32 once and the arithmetic is the same, so an integer-valued float gives the bits
// of the int64 form.
template <typename T>
__global__ void timestep_embedding_kernel(const T* __restrict__ t_dev, int rows, const int32_t* __restrict__ step_dev,
                                          int32_t* __restrict__ step_error, float* __restrict__ out, int B, int dim, int flip, float shift) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * dim) return;
    const int j = i % dim, half = dim / 2;
    const float tv = (float)t_dev[table_row(step_dev, rows, step_error)];
    const int kk = j < half ? j : j - half;
    const float f = expf(-9.210340371976184f * (float)kk / ((float)half - shift));
    const float a = tv * f;
    const bool is_cos = flip ? (j < half) : (j >= half);
    out[i] = is_cos ? cosf(a) : sinf(a);
}

// the same for a table of timesteps: row i <- t_dev[i]
template <typename T>
__global__ void timestep_embedding_rows_kernel(const T* __restrict__ t_dev, float* __restrict__ out, int n, int dim, int flip, float shift) {
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

// scale_tab != NULL (pcdm_assemble_input_ex): the LATENT channels are multiplied in fp32 by scale_tab[row * scale_stride + scale_col]
// (scheduler.scale_model_input) before their one rounding to bf16; NULL: pcdm_assemble_input, bit for bit
__global__ void assemble_input_kernel(const float* __restrict__ latents, int N, int rep,
                                      const float* __restrict__ mask, int mask_b, const float* __restrict__ masked,
                                      int masked_b, u16* __restrict__ out, int HW, int cpad, const float* __restrict__ scale_tab,
                                      int scale_stride, int scale_col, int scale_rows, const int32_t* __restrict__ step_dev,
                                      int32_t* __restrict__ step_error) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (b, pixel, octet)
    const int noct = cpad / 8;
    const int64_t total = (int64_t)N * rep * HW * noct;
    if (i >= total) return;
    const float sc = scale_tab ? scale_tab[(int64_t)table_row(step_dev, scale_rows, step_error) * scale_stride + scale_col] : 1.f;
    const int oc = (int)(i % noct);
    const int64_t bp = i / noct;
    const int pix = (int)(bp % HW), b = (int)(bp / HW);
    u16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = oc * 8 + e;
        float v = 0.f;
        const int c0 = mask ? 5 : 4;   // no mask channel: [latents | masked] (the stage-3 refinement input)
        if (c < 4) {
            v = latents[((int64_t)(b % N) * 4 + c) * HW + pix];
            if (scale_tab) v = v * sc;
        } else if (mask && c == 4) v = mask[(int64_t)(mask_b == 1 ? 0 : b) * HW + pix];
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
                                float* __restrict__ eps_out, const float* __restrict__ coef, int rows,
                                const int32_t* __restrict__ step_dev, int32_t* __restrict__ step_error, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // coef NULL (CFG combine only): no table, no row, the flag is not touched
    const float* cf = coef ? coef + 4 * table_row(step_dev, rows, step_error) : nullptr;
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
                                  float* __restrict__ m2, float* __restrict__ last, const float* __restrict__ coef, int rows,
                                  const int32_t* __restrict__ step_dev, int32_t* __restrict__ step_error, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* c = coef + 12 * table_row(step_dev, rows, step_error);
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
                                  const float* __restrict__ noise_all, const float* __restrict__ coef, int rows,
                                  const int32_t* __restrict__ step_dev, int32_t* __restrict__ step_error, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int st = table_row(step_dev, rows, step_error);
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

// Euler / Euler-ancestral / LMS / PNDM (PLMS) steps as ONE elementwise kernel on five static fp32 state slots: every one of them is linear in
// (x, a saved sample xs, eps, three older eps h1..h3, noise) with host-known scalars, row `row` of a DEVICE table (include/pcdm.h,
// PCDM_MS_*).  Per element, with e the CFG-combined eps (fmaf(g, e_cond - e_uncond, e_uncond), as the neighbours under -ffp-contract=fast):
//   x' = fma(c_z, z, fma(c_3, h3, fma(c_2, h2, fma(c_1, h1, fma(c_0, e, fma(c_s, xs, c_x * x))))))     (one product, then FUSED multiply-adds in
//        this order; the z term only when a noise table is given and c_z != 0)
//   save != 0: xs <- x (old);  push != 0: h3 <- h2, h2 <- h1, h1 <- e;  x <- x'
// Every element is owned by one lane (no atomics).  Lanes [0, n / 4) take four consecutive elements (16-byte accesses where the address
// allows, e.g. not on the second CFG half or a noise row of an n that is no multiple of 4), lanes [n / 4, n / 4 + n % 4) one tail element each.
struct MsRow { float cx, cs, c0, c1, c2, c3, cz; bool save, push; };
__device__ __forceinline__ float ms_update(const MsRow& r, float x, float xs, float e, float a1, float a2, float a3, float z, bool noisy) {
    float v = r.cx * x;
    v = fmaf(r.cs, xs, v);
    v = fmaf(r.c0, e, v);
    v = fmaf(r.c1, a1, v);
    v = fmaf(r.c2, a2, v);
    v = fmaf(r.c3, a3, v);
    if (noisy) v = fmaf(r.cz, z, v);
    return v;
}
__device__ __forceinline__ f32x4 ms_load4(const float* p) {
    if (((uintptr_t)p & 15) == 0) return *(const f32x4*)p;
    return f32x4{p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ void ms_store4(float* p, f32x4 v) {
    if (((uintptr_t)p & 15) == 0) { *(f32x4*)p = v; return; }
    p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
}
__global__ void multistep_step_kernel(const float* __restrict__ eps, int cfg, float g, float* __restrict__ x, float* __restrict__ xs,
                                      float* __restrict__ h1, float* __restrict__ h2, float* __restrict__ h3,
                                      const float* __restrict__ noise_all, const float* __restrict__ coef, int rows,
                                      const int32_t* __restrict__ step_dev, int32_t* __restrict__ step_error, int64_t n) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nvec = n >> 2;
    if (t >= nvec + (n & 3)) return;
    const int st = table_row(step_dev, rows, step_error);
    const float* c = coef + (int64_t)PCDM_MS_ROW * st;
    const MsRow r{c[PCDM_MS_CX], c[PCDM_MS_CS], c[PCDM_MS_C0], c[PCDM_MS_C1], c[PCDM_MS_C2], c[PCDM_MS_C3], c[PCDM_MS_CZ],
                  c[PCDM_MS_SAVE] != 0.f, c[PCDM_MS_PUSH] != 0.f};
    const bool noisy = noise_all && r.cz != 0.f;
    const float* z = noise_all ? noise_all + (int64_t)st * n : nullptr;
    if (t < nvec) {
        const int64_t i = t * 4;
        f32x4 e = ms_load4(eps + i);
        if (cfg) {
            const f32x4 ec = ms_load4(eps + n + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) e[k] = fmaf(g, ec[k] - e[k], e[k]);
        }
        const f32x4 xv = ms_load4(x + i), sv = ms_load4(xs + i), a1 = ms_load4(h1 + i), a2 = ms_load4(h2 + i), a3 = ms_load4(h3 + i);
        f32x4 zv = {0.f, 0.f, 0.f, 0.f};
        if (noisy) zv = ms_load4(z + i);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = ms_update(r, xv[k], sv[k], e[k], a1[k], a2[k], a3[k], zv[k], noisy);
        if (r.save) ms_store4(xs + i, xv);
        if (r.push) {
            ms_store4(h3 + i, a2);
            ms_store4(h2 + i, a1);
            ms_store4(h1 + i, e);
        }
        ms_store4(x + i, o);
    } else {
        const int64_t i = nvec * 4 + (t - nvec);
        float e = eps[i];
        if (cfg) e = fmaf(g, eps[n + i] - e, e);
        const float xv = x[i], a1 = h1[i], a2 = h2[i];
        const float o = ms_update(r, xv, xs[i], e, a1, a2, h3[i], noisy ? z[i] : 0.f, noisy);
        if (r.save) xs[i] = xv;
        if (r.push) {
            h3[i] = a2;
            h2[i] = a1;
            h1[i] = e;
        }
        x[i] = o;
    }
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
                                       const float* __restrict__ noise_all, const float* __restrict__ coef, int rows,
                                       const int32_t* __restrict__ step_dev, int32_t* __restrict__ step_error, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int st = table_row(step_dev, rows, step_error);
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

__global__ void advance_step_kernel(int32_t* step) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *step += 1;
}
}  // namespace

extern "C" int pcdm_version(void) { return PCDM_ABI_VERSION; }   // 6: every step-indexed table read takes its row count and an error flag (include/pcdm.h)
extern "C" int pcdm_is_emulator(void) {
#ifdef PCDM_EMU
    return 1;
#else
    return 0;
#endif
}

extern "C" int pcdm_timestep_embedding(const int64_t* t_dev, int rows, const int32_t* step_dev, int32_t* step_error, float* out, int B,
                                       int dim, int flip_sin_to_cos, float shift, pcdm_stream_t s) {
    if (!t_dev || !out || B <= 0 || dim <= 0 || dim % 2 || rows < 1 || ((uintptr_t)step_error & 3)) return -1;
    PCDM_LAUNCH(timestep_embedding_kernel<int64_t>, grid1d((int64_t)B * dim, 256), dim3(256), 0, (hipStream_t)s, t_dev, rows, step_dev,
                step_error, out, B, dim, flip_sin_to_cos, shift);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_timestep_embedding_f32(const float* t_dev, int rows, const int32_t* step_dev, int32_t* step_error, float* out, int B,
                                           int dim, int flip_sin_to_cos, float shift, pcdm_stream_t s) {
    if (!t_dev || !out || B <= 0 || dim <= 0 || dim % 2 || rows < 1 || ((uintptr_t)step_error & 3)) return -1;
    PCDM_LAUNCH(timestep_embedding_kernel<float>, grid1d((int64_t)B * dim, 256), dim3(256), 0, (hipStream_t)s, t_dev, rows, step_dev,
                step_error, out, B, dim, flip_sin_to_cos, shift);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_timestep_embedding_rows(const int64_t* t_dev, int n, float* out, int dim, int flip_sin_to_cos, float shift, pcdm_stream_t s) {
    if (!t_dev || !out || n <= 0 || dim <= 0 || dim % 2) return -1;
    PCDM_LAUNCH(timestep_embedding_rows_kernel<int64_t>, grid1d((int64_t)n * dim, 256), dim3(256), 0, (hipStream_t)s, t_dev, out, n, dim, flip_sin_to_cos, shift);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_timestep_embedding_rows_f32(const float* t_dev, int n, float* out, int dim, int flip_sin_to_cos, float shift, pcdm_stream_t s) {
    if (!t_dev || !out || n <= 0 || dim <= 0 || dim % 2) return -1;
    PCDM_LAUNCH(timestep_embedding_rows_kernel<float>, grid1d((int64_t)n * dim, 256), dim3(256), 0, (hipStream_t)s, t_dev, out, n, dim, flip_sin_to_cos, shift);
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
                masked, masked_b, (u16*)out, h * w, cpad, (const float*)nullptr, 0, 0, 1, (const int32_t*)nullptr, (int32_t*)nullptr);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_assemble_input_ex(const float* latents, int N, int rep, const float* mask, int mask_b,
                                      const float* masked, int masked_b, void* out, int h, int w, int cpad,
                                      const float* scale_tab, int scale_stride, int scale_col, int scale_rows,
                                      const int32_t* step_dev, int32_t* step_error, pcdm_stream_t s) {
    if (!latents || !masked || !out || N <= 0 || rep <= 0 || h <= 0 || w <= 0 || cpad % 8 || cpad < 16) return -1;
    if (scale_tab && (scale_rows < 1 || scale_stride < 1 || scale_col < 0 || scale_col >= scale_stride || ((uintptr_t)step_error & 3))) return -1;
    const int64_t total = (int64_t)N * rep * h * w * (cpad / 8);
    PCDM_LAUNCH(assemble_input_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, latents, N, rep, mask, mask_b,
                masked, masked_b, (u16*)out, h * w, cpad, scale_tab, scale_stride, scale_col, scale_rows, step_dev, step_error);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_nchw_f32_to_nhwc_bf16(const float* x, void* y, int B, int C, int Cpad, int HW, pcdm_stream_t s) {
    if (!x || !y || B <= 0 || C <= 0 || HW <= 0 || Cpad % 8 || Cpad < C) return -1;
    const int64_t total = (int64_t)B * HW * (Cpad / 8);
    PCDM_LAUNCH(nchw_to_nhwc_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, x, (u16*)y, C, Cpad, HW, total);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_nhwc_bf16_to_nchw_f32(const void* x, float* y, int B, int C, int HW, pcdm_stream_t s) {
    if (!x || !y || B <= 0 || C <= 0 || HW <= 0) return -1;
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
                             float* eps_out, const float* coef, int rows, const int32_t* step_dev, int32_t* step_error, int64_t n,
                             pcdm_stream_t s) {
    if (!eps || n <= 0 || (x_prev && (!x || !coef))) return -1;
    if (coef && (rows < 1 || ((uintptr_t)step_error & 3))) return -1;   // coef NULL: no table is read, rows / step_error are ignored
    PCDM_LAUNCH(cfg_step_kernel, grid1d(n, 256), dim3(256), 0, (hipStream_t)s, eps, cfg, g, x, noise, x_prev, eps_out,
                coef, rows, step_dev, step_error, n);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_unipc_step(const float* eps, int cfg, float g, float* x, float* m1, float* m2, float* last, const float* coef,
                               int rows, const int32_t* step_dev, int32_t* step_error, int64_t n, pcdm_stream_t s) {
    if (!eps || !x || !m1 || !m2 || !last || !coef || n <= 0 || rows < 1 || ((uintptr_t)step_error & 3)) return -1;
    PCDM_LAUNCH(unipc_step_kernel, grid1d(n, 256), dim3(256), 0, (hipStream_t)s, eps, cfg, g, x, m1, m2, last, coef, rows, step_dev,
                step_error, n);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_dpmpp_step(const float* eps, int cfg, float g, float* x, float* m1, const float* noise_all, const float* coef,
                               int rows, const int32_t* step_dev, int32_t* step_error, int64_t n, pcdm_stream_t s) {
    if (!eps || !x || !m1 || !coef || n <= 0 || rows < 1 || ((uintptr_t)step_error & 3)) return -1;
    PCDM_LAUNCH(dpmpp_step_kernel, grid1d(n, 256), dim3(256), 0, (hipStream_t)s, eps, cfg, g, x, m1, noise_all, coef, rows, step_dev,
                step_error, n);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_multistep_step(const float* eps, int cfg, float g, float* x, float* xs, float* h1, float* h2, float* h3,
                                   const float* noise_all, const float* coef, int rows, const int32_t* step_dev, int32_t* step_error,
                                   int64_t n, pcdm_stream_t s) {
    if (!eps || !x || !xs || !h1 || !h2 || !h3 || !coef || rows < 1 || n < 1 || ((uintptr_t)step_error & 3)) return -1;
    PCDM_LAUNCH(multistep_step_kernel, grid1d((n >> 2) + (n & 3), 256), dim3(256), 0, (hipStream_t)s, eps, cfg, g, x, xs, h1, h2, h3, noise_all,
                coef, rows, step_dev, step_error, n);
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
                                    int rows, const int32_t* step_dev, int32_t* step_error, int64_t n, pcdm_stream_t s) {
    if (!pred || !x || !coef || n <= 0 || rows < 1 || ((uintptr_t)step_error & 3)) return -1;
    PCDM_LAUNCH(unclip_step_dev_kernel, grid1d(n, 256), dim3(256), 0, (hipStream_t)s, pred, cfg, g, x, noise_all, coef, rows, step_dev,
                step_error, n);
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

// bf16 [rows, ldx] -> e4m3 [rows, ldy] (bytes), y = sat(x * scale); 8 elements per thread (16 B in where x and ldx keep every row 16-byte
// aligned, eight 2-byte loads otherwise; 8 B out); columns >= cols of a row (up to cols_pad) are written as zero: the K / V^T operands of
// pcdm_flash_attn_fp8
__global__ __launch_bounds__(256) void quantize_fp8_kernel(const u16* __restrict__ x, uint8_t* __restrict__ y, int64_t rows, int cols,
                                                           int cols_pad, int64_t ldx, int64_t ldy, float scale) {
    const int per_row = cols_pad / 8;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * per_row) return;
    const int64_t r = i / per_row;
    const int c = (int)(i - r * per_row) * 8;
    float v[8];
    if (c + 8 <= cols && (ldx & 7) == 0 && ((uintptr_t)x & 15) == 0) {   // (every row starts 16-byte aligned: base and row stride)
        const u16x8 a = *(const u16x8*)(x + r * ldx + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = bf2f(a[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = c + e < cols ? bf2f(x[r * ldx + c + e]) : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {   // saturate; comparisons, not fminf / fmaxf: those drop a NaN operand, and a NaN must reach the convert (-> 0x7f / 0xff)
        const float t = v[e] * scale;
        v[e] = t > 448.f ? 448.f : (t < -448.f ? -448.f : t);
    }
    u32x2 o = {pack4_fp8(v[0], v[1], v[2], v[3]), pack4_fp8(v[4], v[5], v[6], v[7])};
    *(u32x2*)(y + r * ldy + c) = o;
}

extern "C" int pcdm_quantize_fp8(const void* x, void* y, int64_t rows, int cols, int cols_pad, int64_t ldx, int64_t ldy, float scale,
                                 pcdm_stream_t s) {
    if (!x || !y || rows <= 0 || cols <= 0 || cols_pad < cols || cols_pad % 8 || ldy % 8 || ldy < cols_pad || ldx < cols ||
        ((uintptr_t)y & 7)) return -1;   // (y is stored in 8-byte pieces)
    const int64_t total = rows * (cols_pad / 8);
    PCDM_LAUNCH(quantize_fp8_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, (const u16*)x, (uint8_t*)y, rows, cols, cols_pad,
                ldx, ldy, scale);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_softmax_rows(const float* s_in, void* p_out, int rows, int cols, int64_t ld_s, int64_t ld_p, float scale,
                                 pcdm_stream_t s) {
    if (!s_in || !p_out || rows <= 0 || cols <= 0 || cols > 8192 || ld_s < cols || ld_p < cols) return -1;
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

// An emulator build script from before the evaluation code became units of its own names this file and not those units, and still has to link
// every pcdm_* entry: an emulator build that does not say it compiles them (PCDM_EMU_UNITS, tests/emu/build_emu.py) gets them from here.
#if defined(PCDM_EMU) && !defined(PCDM_EMU_UNITS)
#include "image_metrics.hip"
#include "image_prep.hip"
#include "eval_nets.hip"
#endif
