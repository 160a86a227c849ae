#include "pcdm_device.h"
#include "../../include/pcdm.h"
#include "image_common.h"

// ---- The whole-body pose estimator (mmpose's top-down DWPose-l: CSPNeXt backbone, RTMCC head, SimCC decoding; include/pcdm.h states the network) ----
// Everything that is not a dense convolution: box -> normalised crop, depthwise 5 x 5, the SPP maxima, the channel-attention vector, ScaleNorm, the
// gated-attention core and the SimCC decode; and pcdm_dwpose_forward, the whole schedule as one C call on one workspace.  The convolutions and the
// linears run on pcdm_conv2d_f32_act (eval_nets.hip).  fp32 NHWC, channels in groups of four (one 16-byte load per lane), no atomics, no
// allocation, no host synchronisation; every sum has a fixed order, so reruns are bit-identical and a crop's result does not depend on its place
// in the batch.
namespace {
struct PoseBox { float cx, cy, w, h; };

// GetBBoxCenterScale (padding 1.25) + TopdownAffine's aspect fix, every operation its own fp32 operation
__device__ __forceinline__ PoseBox pose_box(const float* b, int Hin, int Win) {
    PoseBox o;
    o.cx = cv_mul(b[0] + b[2], 0.5f);
    o.cy = cv_mul(b[1] + b[3], 0.5f);
    o.w = cv_mul(b[2] - b[0], 1.25f);
    o.h = cv_mul(b[3] - b[1], 1.25f);
    const float ar = (float)Win / (float)Hin;
    if (o.w > cv_mul(o.h, ar)) o.h = o.w / ar;
    else o.w = cv_mul(o.h, ar);
    return o;
}

// rint, saturated to the int32 range (NaN: the lower bound), as a 64-bit integer
__device__ __forceinline__ int64_t sat_rint(double v) {
    if (!(v >= -2147483648.0)) return -2147483648LL;
    if (v > 2147483647.0) return 2147483647LL;
    return (int64_t)rint(v);
}

// out fp32 NHWC [R2, Hin, Win, 4] (R2 = R or 2 R; channel 3 = 0) <- the 8-bit fixed-point bilinear warp of box r's crop, normalised per channel;
// crops R .. 2 R - 1 are the first R mirrored in x.  One lane per output pixel.
__global__ __launch_bounds__(256) void pose_crop_kernel(const uint8_t* __restrict__ img, int N, int H, int W, const float* __restrict__ boxes,
                                                        const int32_t* __restrict__ index, int R, int Hin, int Win, int64_t total,
                                                        float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over (crop, y, x)
    if (i >= total) return;
    const int x = (int)(i % Win);
    const int64_t t = i / Win;
    const int y = (int)(t % Hin), r2 = (int)(t / Hin);
    const int r = r2 >= R ? r2 - R : r2, xd = r2 >= R ? Win - 1 - x : x;
    const PoseBox b = pose_box(boxes + 4 * r, Hin, Win);
    const int n = index ? index[r] : 0;
    const double inv = (double)b.w / (double)Win;
    const double bx = (double)b.cx - 0.5 * (double)Win * inv, by = (double)b.cy - 0.5 * (double)Hin * inv;
    const int64_t X = (sat_rint(bx * 1024.0) + 16 + sat_rint(inv * (double)xd * 1024.0)) >> 5;
    const int64_t Y = (sat_rint(by * 1024.0) + 16 + sat_rint(inv * (double)y * 1024.0)) >> 5;
    const int64_t sx = X >> 5, sy = Y >> 5;
    const int fx = (int)(X & 31), fy = (int)(Y & 31);
    int acc[3] = {0, 0, 0};
    if ((unsigned)n < (unsigned)N && sx >= -1 && sx < W && sy >= -1 && sy < H) {
        const uint8_t* base = img + (int64_t)n * H * W * 3;
        const int wt[4] = {(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int px = (int)sx + (k & 1), py = (int)sy + (k >> 1);
            if (wt[k] == 0 || (unsigned)px >= (unsigned)W || (unsigned)py >= (unsigned)H) continue;
            const uint8_t* p = base + ((int64_t)py * W + px) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += wt[k] * (int)p[c];
        }
    }
    const float mean[3] = {123.675f, 116.28f, 103.53f}, sd[3] = {58.395f, 57.12f, 57.375f};
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = ((float)((acc[c] + 16384) >> 15) - mean[c]) / sd[c];
    *(f32x4*)(out + i * 4) = o;
}

// Depthwise 5 x 5, pad 2, stride 1, + bias + SiLU.  Bandwidth-bound (25 FMAs per loaded weight vector, no reuse across channels), so not on the
// matrix pipe: one lane = one pixel x four channels, 16-byte loads of the channel vector and of the tap's weights w[(ky 5 + kx)][C], taps in
// (ky, kx) order, taps outside the image skipped.  Neighbouring lanes hold neighbouring channel groups of one pixel: every load of a wave is one
// contiguous run, and the 25-fold reuse of a pixel comes from L1 / L2 (the largest map of the network is 1.7 MB a crop), so no LDS halo.
__global__ __launch_bounds__(256) void dw5_silu_kernel(const float* __restrict__ x, int ldi, const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out, int ldo, int H, int W, int C4, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over (b, y, x, c / 4)
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    int64_t t = i / C4;
    const int64_t pix = t;
    const int px = (int)(t % W);
    t /= W;
    const int py = (int)(t % H), b = (int)(t / H);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 5; ++ky)
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) {
            const int yy = py + ky - 2, xx = px + kx - 2;
            if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
            const f32x4 v = *(const f32x4*)(x + (((int64_t)b * H + yy) * W + xx) * ldi + 4 * c4);
            const f32x4 k = *(const f32x4*)(w + ((int64_t)(ky * 5 + kx) * C4 + c4) * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(v[e], k[e], acc[e]);
        }
    const f32x4 bv = *(const f32x4*)(bias + 4 * c4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float v = acc[e] + bv[e];
        acc[e] = v / (1.0f + expf(-v));
    }
    *(f32x4*)(out + pix * ldo + 4 * c4) = acc;
}

// MaxPool2d(5, stride 1, pad 2): the padding never wins, a NaN does (as torch).  Reads one channel slice, writes another (they may belong to one tensor).
__global__ __launch_bounds__(256) void maxpool5_f32_kernel(const float* x, int ldi, float* out, int ldo, int H, int W, int C4, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over (b, y, x, c / 4)
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    int64_t t = i / C4;
    const int64_t pix = t;
    const int px = (int)(t % W);
    t /= W;
    const int py = (int)(t % H), b = (int)(t / H);
    f32x4 m = *(const f32x4*)(x + pix * ldi + 4 * c4);
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const int yy = py + dy, xx = px + dx;
            if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
            const f32x4 v = *(const f32x4*)(x + (((int64_t)b * H + yy) * W + xx) * ldi + 4 * c4);
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = v[e] > m[e] || v[e] != v[e] ? v[e] : m[e];
        }
    *(f32x4*)(out + pix * ldo + 4 * c4) = m;
}

// ChannelAttention's vector: out[b, n] = hardsigmoid(sum_c w[n, c] x[b, c] + bias[n]), hardsigmoid(v) = clamp(v + 3, 0, 6) / 6.  One wave per
// output: lane l adds the channels l, l + 64, .. in order, then the wave's butterfly.
__global__ __launch_bounds__(256) void fc_hsigmoid_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ out, int C, int total) {
    const int lane = threadIdx.x & 63, o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= total) return;
    const int n = o % C, b = o / C;
    float acc = 0.f;
    for (int c = lane; c < C; c += 64) acc = fmaf(w[(int64_t)n * C + c], x[(int64_t)b * C + c], acc);
    float v = wave_sum(acc) + bias[n] + 3.0f;
    v = v < 0.f ? 0.f : (v > 6.f ? 6.f : v);
    if (lane == 0) out[o] = v / 6.0f;
}

// ScaleNorm: out[row, i] = x / max(|x|_2 scale, eps) * g[0] over the `dim` elements of a row, element i of row (b, k) at x[b bs + k rs + i es] (the
// head's first norm reads the NHWC feature map [B, P, pitch] as [B, K, P] without a transposing pass).  Columns dim .. ldo - 1 of out are zeroed.
// side (or NULL): side[row, i] = x * side_scale[i], the GAU's scaled shortcut.  One wave per row.
__global__ __launch_bounds__(256) void scalenorm_kernel(const float* __restrict__ x, int rows, int64_t bs, int64_t rs, int64_t es, int dim, float scale,
                                                        float eps, const float* __restrict__ g, float* __restrict__ out, int ldo,
                                                        const float* __restrict__ side_scale, float* __restrict__ side, int lds, int total) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= total) return;
    const float* src = x + (int64_t)(row / rows) * bs + (int64_t)(row % rows) * rs;
    float ss = 0.f;
    for (int i = lane; i < dim; i += 64) {
        const float v = src[(int64_t)i * es];
        ss = fmaf(v, v, ss);
    }
    const float norm = sqrtf(wave_sum(ss)) * scale;
    const float d = norm < eps ? eps : norm, gv = g[0];
    for (int i = lane; i < ldo; i += 64) out[(int64_t)row * ldo + i] = i < dim ? src[(int64_t)i * es] / d * gv : 0.f;
    if (side)
        for (int i = lane; i < dim; i += 64) side[(int64_t)row * lds + i] = src[(int64_t)i * es] * side_scale[i];
}

// The gated-attention core of one crop: uv fp32 [B T, 2 e + 128] = SiLU(Linear(h)) split as (u | v | base); q = base gamma[0] + beta[0],
// k = base gamma[1] + beta[1], A = relu(q k^T / sqrt(128))^2, out [B T, e] = u * (A v).  A workgroup owns eight query rows of one crop and 256
// columns of v: q of its rows and then its 8 x T tile of A go through LDS, each A entry one 128-long fmaf chain, each output one T-long chain.
constexpr int kGauS = 128, kGauRows = 8, kGauMaxT = 256;
__global__ __launch_bounds__(256) void gau_core_kernel(const float* __restrict__ uv, int T, int e, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ out) {
    __shared__ float qs[kGauRows][kGauS];
    __shared__ float as[kGauRows][kGauMaxT];
    const int tid = threadIdx.x, i0 = blockIdx.x * kGauRows, b = blockIdx.z, ld = 2 * e + kGauS;
    const float* crop = uv + (int64_t)b * T * ld;
    for (int idx = tid; idx < kGauRows * kGauS; idx += 256) {
        const int i = idx / kGauS, d = idx % kGauS;
        qs[i][d] = i0 + i < T ? fmaf(crop[(int64_t)(i0 + i) * ld + 2 * e + d], gamma[d], beta[d]) : 0.f;
    }
    __syncthreads();
    const float rs = 1.0f / sqrtf((float)kGauS);
    for (int p = tid; p < kGauRows * T; p += 256) {
        const int i = p / T, j = p % T;
        const float* bj = crop + (int64_t)j * ld + 2 * e;
        float acc = 0.f;
        for (int d = 0; d < kGauS; d += 4) {
            const f32x4 v = *(const f32x4*)(bj + d), gm = *(const f32x4*)(gamma + kGauS + d), bt = *(const f32x4*)(beta + kGauS + d);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = fmaf(qs[i][d + q], fmaf(v[q], gm[q], bt[q]), acc);
        }
        const float a = acc * rs, r = a > 0.f ? a : (a != a ? a : 0.f);
        as[i][j] = r * r;
    }
    __syncthreads();
    const int c = blockIdx.y * 256 + tid;
    if (c >= e) return;
    float acc[kGauRows];
#pragma unroll
    for (int i = 0; i < kGauRows; ++i) acc[i] = 0.f;
    for (int j = 0; j < T; ++j) {
        const float vj = crop[(int64_t)j * ld + e + c];
#pragma unroll
        for (int i = 0; i < kGauRows; ++i) acc[i] = fmaf(as[i][j], vj, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < kGauRows; ++i)
        if (i0 + i < T) out[((int64_t)b * T + i0 + i) * e + c] = crop[(int64_t)(i0 + i) * ld + c] * acc[i];
}

// is (v, i) a better maximum than (bv, bi)?  np.argmax's order: a NaN beats every number, the first of equals wins
__device__ __forceinline__ bool simcc_better(float v, int i, float bv, int bi) {
    if (bv != bv) return v != v && i < bi;
    return v != v || v > bv || (v == bv && i < bi);
}

// SimCC decode of keypoint k of box r (one wave each): logits sx fp32 [R2 K, ldx] (nx bins), sy [R2 K, ldy] (ny bins), R2 = 2 R with flip: the
// flipped crop's output for keypoint k is row flip_idx[k] of crop R + r, its x bins reversed; merged = 0.5 (plain + flipped).  loc = the first
// maximum per axis; score = max_x > max_y ? max_y : max_x; loc = -1 on both axes where score <= 0; keypoint = (loc / 2) / (Win, Hin) * (w, h) +
// c - 0.5 (w, h) in fp32, every operation its own.
__global__ __launch_bounds__(256) void simcc_decode_kernel(const float* __restrict__ sx, int ldx, int nx, const float* __restrict__ sy, int ldy, int ny,
                                                           int R, int K, int flip, const int32_t* __restrict__ flip_idx, const float* __restrict__ boxes,
                                                           int Hin, int Win, float* __restrict__ kp, float* __restrict__ score) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R * K) return;
    const int r = row / K, k = row % K;
    int kf = k;
    if (flip && flip_idx) {
        const int f = flip_idx[k];
        if ((unsigned)f < (unsigned)K) kf = f;
    }
    float best[2];
    int loc[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int n = a ? ny : nx, ld = a ? ldy : ldx;
        const float* p = (a ? sy : sx) + (int64_t)row * ld;
        const float* f = (a ? sy : sx) + ((int64_t)(R + r) * K + kf) * ld;
        float bv = -__builtin_inff();
        int bi = 0x7fffffff;
        for (int i = lane; i < n; i += 64) {
            const float v = flip ? 0.5f * (p[i] + f[a ? i : n - 1 - i]) : p[i];
            if (simcc_better(v, i, bv, bi)) { bv = v; bi = i; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ov = __shfl_xor(bv, m, 64);
            const int oi = __shfl_xor(bi, m, 64);
            if (simcc_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        best[a] = bv;
        loc[a] = bi;
    }
    if (lane != 0) return;
    const float sc = best[0] > best[1] ? best[1] : best[0];
    const bool drop = sc <= 0.f;
    const PoseBox bx = pose_box(boxes + 4 * r, Hin, Win);
    const float lx = (drop ? -1.0f : (float)loc[0]) / 2.0f, ly = (drop ? -1.0f : (float)loc[1]) / 2.0f;
    kp[(int64_t)row * 2] = cv_mul(lx / (float)Win, bx.w) + bx.cx - cv_mul(0.5f, bx.w);
    kp[(int64_t)row * 2 + 1] = cv_mul(ly / (float)Hin, bx.h) + bx.cy - cv_mul(0.5f, bx.h);
    score[row] = sc;
}

inline bool slice_ok(int C, int ld, int off) { return C > 0 && C % 4 == 0 && ld % 4 == 0 && off >= 0 && off % 4 == 0 && ld >= C && off <= ld - C; }
}  // namespace

extern "C" int pcdm_pose_crop(const void* images, int N, int H, int W, const float* boxes, const int32_t* image_index, int R, int flip, int Hin, int Win,
                              float* out, pcdm_stream_t s) {
    if (!images || !boxes || !out || N <= 0 || H <= 0 || W <= 0 || R <= 0 || Hin <= 0 || Win <= 0 || Hin > 4096 || Win > 4096 || ((uintptr_t)out & 15))
        return -1;
    const int64_t total = (int64_t)R * (flip ? 2 : 1) * Hin * Win;
    if ((int64_t)N * H * W * 3 >= (int64_t)1 << 31 || total * 4 >= (int64_t)1 << 31) return -1;
    PCDM_LAUNCH(pose_crop_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, (const uint8_t*)images, N, H, W, boxes, image_index, R, Hin, Win,
                total, out);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_dwconv5_silu_f32(const float* x, int B, int H, int W, int C, int in_pitch, int in_offset, const float* w, const float* bias, float* out,
                                     int out_pitch, int out_offset, pcdm_stream_t s) {
    if (!x || !w || !bias || !out || B <= 0 || H <= 0 || W <= 0 || !slice_ok(C, in_pitch, in_offset) || !slice_ok(C, out_pitch, out_offset)) return -1;
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)out) & 15) return -1;
    if (x == out && in_pitch == out_pitch && in_offset < out_offset + C && out_offset < in_offset + C) return -1;   // a pixel's neighbours would be read after they were rewritten
    if ((int64_t)B * H * W * in_pitch >= (int64_t)1 << 31 || (int64_t)B * H * W * out_pitch >= (int64_t)1 << 31) return -1;
    const int64_t total = (int64_t)B * H * W * (C / 4);
    PCDM_LAUNCH(dw5_silu_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, x + in_offset, in_pitch, w, bias, out + out_offset, out_pitch, H, W,
                C / 4, total);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_maxpool5_f32(const float* x, int B, int H, int W, int C, int in_pitch, int in_offset, float* out, int out_pitch, int out_offset,
                                 pcdm_stream_t s) {
    if (!x || !out || B <= 0 || H <= 0 || W <= 0 || !slice_ok(C, in_pitch, in_offset) || !slice_ok(C, out_pitch, out_offset)) return -1;
    if (((uintptr_t)x | (uintptr_t)out) & 15) return -1;
    if (x == out && in_pitch == out_pitch && in_offset < out_offset + C && out_offset < in_offset + C) return -1;   // overlapping slices of one tensor
    if ((int64_t)B * H * W * in_pitch >= (int64_t)1 << 31 || (int64_t)B * H * W * out_pitch >= (int64_t)1 << 31) return -1;
    const int64_t total = (int64_t)B * H * W * (C / 4);
    PCDM_LAUNCH(maxpool5_f32_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, x + in_offset, in_pitch, out + out_offset, out_pitch, H, W, C / 4,
                total);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_fc_hsigmoid_f32(const float* x, int B, int C, const float* w, const float* bias, float* out, pcdm_stream_t s) {
    if (!x || !w || !bias || !out || B <= 0 || C <= 0 || (int64_t)B * C >= (int64_t)1 << 28 || (int64_t)C * C >= (int64_t)1 << 31) return -1;
    PCDM_LAUNCH(fc_hsigmoid_kernel, grid1d((int64_t)B * C, 4), dim3(256), 0, (hipStream_t)s, x, w, bias, out, C, B * C);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_scalenorm_f32(const float* x, int B, int rows, int dim, int64_t batch_stride, int64_t row_stride, int64_t elem_stride, float eps,
                                  const float* g, float* out, int out_pitch, const float* side_scale, float* side_out, int side_pitch, pcdm_stream_t s) {
    if (!x || !g || !out || B <= 0 || rows <= 0 || dim <= 0 || out_pitch < dim || batch_stride < 0 || row_stride < 0 || elem_stride <= 0) return -1;
    if ((side_out != nullptr) != (side_scale != nullptr) || (side_out && side_pitch < dim)) return -1;
    const int64_t total = (int64_t)B * rows;
    const int64_t last = (B - 1) * batch_stride + (rows - 1) * row_stride + (dim - 1) * elem_stride;
    if (total >= (int64_t)1 << 28 || last >= (int64_t)1 << 31 || total * out_pitch >= (int64_t)1 << 31 || (side_out && total * side_pitch >= (int64_t)1 << 31))
        return -1;
    PCDM_LAUNCH(scalenorm_kernel, grid1d(total, 4), dim3(256), 0, (hipStream_t)s, x, rows, batch_stride, row_stride, elem_stride, dim,
                (float)(1.0 / sqrt((double)dim)), eps, g, out, out_pitch, side_scale, side_out, side_pitch, (int)total);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_gau_core_f32(const float* uv, int B, int T, int e, const float* gamma, const float* beta, float* out, pcdm_stream_t s) {
    if (!uv || !gamma || !beta || !out || B <= 0 || B > 65535 || T <= 0 || T > kGauMaxT || e <= 0 || e % 4 || e > 1 << 16) return -1;
    if (((uintptr_t)uv | (uintptr_t)gamma | (uintptr_t)beta) & 15) return -1;
    if ((int64_t)B * T * (2 * e + kGauS) >= (int64_t)1 << 31) return -1;
    PCDM_LAUNCH(gau_core_kernel, dim3((T + kGauRows - 1) / kGauRows, (e + 255) / 256, B), dim3(256), 0, (hipStream_t)s, uv, T, e, gamma, beta, out);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_simcc_decode(const float* simcc_x, int x_pitch, int x_bins, const float* simcc_y, int y_pitch, int y_bins, int R, int K, int flip,
                                 const int32_t* flip_idx, const float* boxes, int Hin, int Win, float* keypoints, float* scores, pcdm_stream_t s) {
    if (!simcc_x || !simcc_y || !boxes || !keypoints || !scores || R <= 0 || K <= 0 || x_bins <= 0 || y_bins <= 0 || x_pitch < x_bins || y_pitch < y_bins ||
        Hin <= 0 || Win <= 0 || (flip && !flip_idx))
        return -1;
    const int64_t rows = (int64_t)R * K * (flip ? 2 : 1);
    if (rows * x_pitch >= (int64_t)1 << 31 || rows * y_pitch >= (int64_t)1 << 31) return -1;
    PCDM_LAUNCH(simcc_decode_kernel, grid1d((int64_t)R * K, 4), dim3(256), 0, (hipStream_t)s, simcc_x, x_pitch, x_bins, simcc_y, y_pitch, y_bins, R, K,
                flip ? 1 : 0, flip_idx, boxes, Hin, Win, keypoints, scores);
    PCDM_CHECK_LAUNCH();
    return 0;
}

// ---- the whole schedule as one C call (as pcdm_inception_features): crop -> backbone -> head -> decode on one caller-owned workspace ------------
namespace {
constexpr int kDwHidden = 256, kDwE = 512;                      // RTMCCHead: hidden_dims, hidden_dims x expansion_factor
struct DwLayout {
    // byte offsets: crops | x0, x1 (the running tensor, ping-pong) | cat | t, u (a block's intermediates) | pool, att | the head's tensors
    int64_t crop, x[2], cat, t, u, pool, att, f, tok, x1, hn, sc, uv, core, x2, logits, total;
    struct { const char* name; int64_t off, bytes; } ent[17];   // every buffer in offset order (pcdm_dwpose_ws_layout)
    int n_ent;
};
inline int64_t dw_align(int64_t elems) { return (elems * (int64_t)sizeof(float) + 255) / 256 * 256; }
inline bool dwpose_cfg_ok(const pcdm_dwpose_config* c) {
    if (!c || c->Hin <= 0 || c->Win <= 0 || c->Hin % 32 || c->Win % 32 || c->Hin > 4096 || c->Win > 4096 || c->K <= 0 || c->K > kGauMaxT) return false;
    if (c->stem <= 0 || c->stem % 8 || c->n_stages != 4) return false;
    for (int s = 0; s < 4; ++s)
        if (c->out[s] <= 0 || c->out[s] % 8 || c->blocks[s] <= 0 || c->blocks[s] > 64) return false;
    return true;
}
inline bool dwpose_layout(const pcdm_dwpose_config* c, int R, int flip, DwLayout* o) {
    if (!dwpose_cfg_ok(c) || R <= 0 || R > 4096) return false;
    const int64_t B = (int64_t)R * (flip ? 2 : 1);
    int64_t h = c->Hin / 2, w = c->Win / 2;
    int64_t x = B * h * w * c->stem, cat = 0, t = 0, cmax = 0;
    for (int s = 0; s < 4; ++s) {
        h /= 2; w /= 2;
        const int64_t mid = c->out[s] / 2, px = B * h * w;
        if (px * c->out[s] > x) x = px * c->out[s];
        if (px * (c->spp[s] ? 4 : 2) * mid > cat) cat = px * (c->spp[s] ? 4 : 2) * mid;
        if (px * mid > t) t = px * mid;
        if (c->out[s] > cmax) cmax = c->out[s];
    }
    const int64_t P = h * w, rows = B * c->K, bins = 2 * (int64_t)c->Win + 2 * (int64_t)c->Hin;
    if (x >= (int64_t)1 << 31 || cat >= (int64_t)1 << 31 || B * c->Hin * c->Win * 4 >= (int64_t)1 << 31 || rows * bins >= (int64_t)1 << 31) return false;
    int64_t at = 0;
    const int64_t redzone = pcdm_get_workspace_redzone();   // (test hook: bytes left unused behind every buffer; 0 in product use)
    o->n_ent = 0;
    auto take = [&](const char* name, int64_t elems) {
        const int64_t here = at;
        o->ent[o->n_ent++] = {name, here, dw_align(elems)};
        at += dw_align(elems) + redzone;
        return here;
    };
    o->crop = take("crop", B * c->Hin * c->Win * 4);
    o->x[0] = take("x0", x); o->x[1] = take("x1", x);
    o->cat = take("cat", cat); o->t = take("t", t); o->u = take("u", t);
    o->pool = take("pool", B * cmax); o->att = take("att", B * cmax);
    o->f = take("f", B * P * c->K); o->tok = take("tok", rows * ((P + 3) / 4 * 4));
    o->x1 = take("head.x1", rows * kDwHidden); o->hn = take("head.hn", rows * kDwHidden); o->sc = take("head.sc", rows * kDwHidden);
    o->uv = take("head.uv", rows * (2 * kDwE + kGauS)); o->core = take("head.core", rows * kDwE); o->x2 = take("head.x2", rows * kDwHidden);
    o->logits = take("logits", rows * bins);
    o->total = at;
    return true;
}
}  // namespace

extern "C" int64_t pcdm_dwpose_ws_bytes(const pcdm_dwpose_config* cfg, int R, int flip) {
    DwLayout lay;
    return dwpose_layout(cfg, R, flip, &lay) ? lay.total : -1;
}

extern "C" int pcdm_dwpose_ws_layout(const pcdm_dwpose_config* cfg, int R, int flip, int index, const char** name, int64_t* offset, int64_t* bytes) {
    DwLayout lay;
    if (!dwpose_layout(cfg, R, flip, &lay)) return -1;
    if (index == -1) return lay.n_ent;
    if (index < 0 || index >= lay.n_ent) return -1;
    if (name) *name = lay.ent[index].name;
    if (offset) *offset = lay.ent[index].off;
    if (bytes) *bytes = lay.ent[index].bytes;
    return lay.n_ent;
}

extern "C" int pcdm_dwpose_forward(const void* images, int N, int H, int W, const float* boxes, const int32_t* image_index, int R, int flip,
                                   const pcdm_dwpose_config* cfg, const pcdm_dwpose_weights* wts, float* keypoints, float* scores, void* ws,
                                   int64_t ws_bytes, pcdm_stream_t s) {
    DwLayout lay;
    if (!images || !boxes || !wts || !keypoints || !scores || !ws || ((uintptr_t)ws & 15) || !dwpose_layout(cfg, R, flip, &lay) || ws_bytes < lay.total)
        return -1;
    int n_conv = 3 + 5, n_dw = 0;                                  // stem; the head's five
    for (int st = 0; st < 4; ++st) {
        n_conv += 4 + (cfg->spp[st] ? 2 : 0) + 2 * cfg->blocks[st];
        n_dw += cfg->blocks[st];
    }
    if (!wts->conv_w || !wts->conv_b || !wts->dw_w || !wts->dw_b || wts->n_conv != n_conv || wts->n_dw != n_dw || !wts->mlp_g || !wts->ln_g ||
        !wts->gamma || !wts->beta || !wts->res_scale || (flip && !wts->flip_idx) || N <= 0 || H <= 0 || W <= 0)
        return -1;
    for (int i = 0; i < n_conv; ++i)
        if (!wts->conv_w[i] || !wts->conv_b[i]) return -1;
    for (int i = 0; i < n_dw; ++i)
        if (!wts->dw_w[i] || !wts->dw_b[i]) return -1;
    for (int st = 0; st < 4; ++st)
        if (!wts->fc_w[st] || !wts->fc_b[st]) return -1;
    char* base = (char*)ws;
    auto buf = [&](int64_t off) { return (float*)(base + off); };
    const int B = R * (flip ? 2 : 1), K = cfg->K, silu = 2;
    int ci = 0, di = 0, rc;
    // conv: the next packed convolution of the schedule, x [B, h, w, cin of pitch ldi] -> channels [off, off + cout) of out [B, ho, wo, ldo]
    auto conv = [&](const float* x, int b, int h, int w, int cin, int ldi, int cout, int k, int stride, int act, const float* res, int ldr,
                    const float* ascale, float* out, int ldo, int off) {
        const int i = ci++;
        return pcdm_conv2d_f32_act(x, b, h, w, cin, ldi, 0, wts->conv_w[i], wts->conv_b[i], cout, k, k, stride, k / 2, k / 2, act, res, ldr, 0, ascale, out,
                                   ldo, off, s);
    };
    rc = pcdm_pose_crop(images, N, H, W, boxes, image_index, R, flip, cfg->Hin, cfg->Win, buf(lay.crop), s);
    if (rc) return rc;
    int h = cfg->Hin / 2, w = cfg->Win / 2, cur = 0, c = cfg->stem;
    if ((rc = conv(buf(lay.crop), B, cfg->Hin, cfg->Win, 4, 4, c / 2, 3, 2, silu, nullptr, 0, nullptr, buf(lay.x[0]), c / 2, 0))) return rc;
    if ((rc = conv(buf(lay.x[0]), B, h, w, c / 2, c / 2, c / 2, 3, 1, silu, nullptr, 0, nullptr, buf(lay.x[1]), c / 2, 0))) return rc;
    if ((rc = conv(buf(lay.x[1]), B, h, w, c / 2, c / 2, c, 3, 1, silu, nullptr, 0, nullptr, buf(lay.x[0]), c, 0))) return rc;
    for (int st = 0; st < 4; ++st) {
        const int co = cfg->out[st], mid = co / 2;
        float* cat = buf(lay.cat);
        if ((rc = conv(buf(lay.x[cur]), B, h, w, c, c, co, 3, 2, silu, nullptr, 0, nullptr, buf(lay.x[cur ^ 1]), co, 0))) return rc;
        cur ^= 1; h /= 2; w /= 2; c = co;
        if (cfg->spp[st]) {
            if ((rc = conv(buf(lay.x[cur]), B, h, w, c, c, mid, 1, 1, silu, nullptr, 0, nullptr, cat, 4 * mid, 0))) return rc;
            for (int j = 0; j < 3; ++j)
                if ((rc = pcdm_maxpool5_f32(cat, B, h, w, mid, 4 * mid, j * mid, cat, 4 * mid, (j + 1) * mid, s))) return rc;
            if ((rc = conv(cat, B, h, w, 4 * mid, 4 * mid, co, 1, 1, silu, nullptr, 0, nullptr, buf(lay.x[cur ^ 1]), co, 0))) return rc;
            cur ^= 1;
        }
        if ((rc = conv(buf(lay.x[cur]), B, h, w, c, c, mid, 1, 1, silu, nullptr, 0, nullptr, cat, 2 * mid, 0))) return rc;
        if ((rc = conv(buf(lay.x[cur]), B, h, w, c, c, mid, 1, 1, silu, nullptr, 0, nullptr, cat, 2 * mid, mid))) return rc;
        for (int b = 0; b < cfg->blocks[st]; ++b) {
            if ((rc = conv(cat, B, h, w, mid, 2 * mid, mid, 3, 1, silu, nullptr, 0, nullptr, buf(lay.t), mid, 0))) return rc;
            if ((rc = pcdm_dwconv5_silu_f32(buf(lay.t), B, h, w, mid, mid, 0, wts->dw_w[di], wts->dw_b[di], buf(lay.u), mid, 0, s))) return rc;
            ++di;
            if ((rc = conv(buf(lay.u), B, h, w, mid, mid, mid, 1, 1, silu, cfg->identity[st] ? cat : nullptr, 2 * mid, nullptr, cat, 2 * mid, 0))) return rc;
        }
        if ((rc = pcdm_global_avgpool_f32(cat, B, h * w, 2 * mid, buf(lay.pool), s))) return rc;
        if ((rc = pcdm_fc_hsigmoid_f32(buf(lay.pool), B, 2 * mid, wts->fc_w[st], wts->fc_b[st], buf(lay.att), s))) return rc;
        if ((rc = conv(cat, B, h, w, 2 * mid, 2 * mid, co, 1, 1, silu, nullptr, 0, buf(lay.att), buf(lay.x[cur ^ 1]), co, 0))) return rc;
        cur ^= 1;
    }
    const int P = h * w, P4 = (P + 3) / 4 * 4, rows = B * K, bins = 2 * cfg->Win + 2 * cfg->Hin, ld_uv = 2 * kDwE + kGauS;
    if ((rc = conv(buf(lay.x[cur]), B, h, w, c, c, K, 7, 1, 0, nullptr, 0, nullptr, buf(lay.f), K, 0))) return rc;
    if ((rc = pcdm_scalenorm_f32(buf(lay.f), B, K, P, (int64_t)P * K, 1, K, 1e-5f, wts->mlp_g, buf(lay.tok), P4, nullptr, nullptr, 0, s))) return rc;
    if ((rc = conv(buf(lay.tok), 1, 1, rows, P4, P4, kDwHidden, 1, 1, 0, nullptr, 0, nullptr, buf(lay.x1), kDwHidden, 0))) return rc;
    if ((rc = pcdm_scalenorm_f32(buf(lay.x1), 1, rows, kDwHidden, 0, kDwHidden, 1, 1e-5f, wts->ln_g, buf(lay.hn), kDwHidden, wts->res_scale, buf(lay.sc),
                                 kDwHidden, s)))
        return rc;
    if ((rc = conv(buf(lay.hn), 1, 1, rows, kDwHidden, kDwHidden, ld_uv, 1, 1, silu, nullptr, 0, nullptr, buf(lay.uv), ld_uv, 0))) return rc;
    if ((rc = pcdm_gau_core_f32(buf(lay.uv), B, K, kDwE, wts->gamma, wts->beta, buf(lay.core), s))) return rc;
    if ((rc = conv(buf(lay.core), 1, 1, rows, kDwE, kDwE, kDwHidden, 1, 1, 0, buf(lay.sc), kDwHidden, nullptr, buf(lay.x2), kDwHidden, 0))) return rc;
    if ((rc = conv(buf(lay.x2), 1, 1, rows, kDwHidden, kDwHidden, bins, 1, 1, 0, nullptr, 0, nullptr, buf(lay.logits), bins, 0))) return rc;
    return pcdm_simcc_decode(buf(lay.logits), bins, 2 * cfg->Win, buf(lay.logits) + 2 * cfg->Win, bins, 2 * cfg->Hin, R, K, flip, wts->flip_idx, boxes,
                             cfg->Hin, cfg->Win, keypoints, scores, s);
}
