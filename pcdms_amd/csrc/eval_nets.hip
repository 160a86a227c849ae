#include "pcdm_device.h"
#include "../../include/pcdm.h"
#include "image_common.h"

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
    // pcdm_conv2d_f32_act only (the EXT instance of the kernel): x = channel 0 of the input slice of an NHWC tensor with ldi channels per pixel;
    // relu = the activation selector (0 none, 1 ReLU, 2 SiLU); res (or NULL): pixel m, channel n at res[m * ldr + n], added after the activation;
    // ascale (or NULL): fp32 [B, Cin], the A operand of image b, input channel c is x * ascale[b * Cin + c]
    int ldi;
    const float* res;
    int ldr;
    const float* ascale;
};

// One wave = a 32 x 64 output tile (2 x 4 accumulators of 16 x 16: eight independent MFMA chains), four waves along M per workgroup, operands
// straight from global memory / L2 (the whole LPIPS call is a few GFLOP; no LDS stage).  Per 16 k: lane (r, g) loads the 16 bytes
// k0 + 4g .. + 3 of its two rows' patches -- Cin % 4 == 0, so a fragment never straddles a tap and an out-of-image tap is one zero fragment,
// not a clamped read -- and of its four weight columns, then runs four MFMA steps per accumulator (mfma_f32_16x16x4_quad).
// The tap (ky, kx, c) of a lane advances by 16 channels per step without a division.  M and N tails: rows >= M load zeros and are not stored,
// 16-column sub-tiles beyond Npad and the second row block of a tile that ends in the first are skipped (wave-uniform).
// EXT = false: pcdm_conv2d_f32 / _ex exactly as they were (a tight input, bias + optional ReLU).  EXT = true: the extras of pcdm_conv2d_f32_act; the
// k order, the fragments and the accumulation are the same, so with every extra off the two instances give the same bits.
template <bool EXT>
__global__ __launch_bounds__(256) void conv_f32_kernel(ConvF32 p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int m0 = (blockIdx.x * 4 + wave) * 32, n0 = blockIdx.y * 64;
    if (m0 >= p.M) return;
    const int nsub = imin(4, (p.Npad - n0) / 16);
    const bool two = m0 + 16 < p.M;
    const float* xb[2];
    const float* sc[2];
    int iy0[2], ix0[2];
    bool valid[2];
    const int ldi = EXT ? p.ldi : p.Cin;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int m = m0 + 16 * t + r;
        valid[t] = m < p.M;
        const int mm = valid[t] ? m : 0;
        const int b = mm / (p.Ho * p.Wo), q = mm - b * p.Ho * p.Wo;
        const int oy = q / p.Wo, ox = q - oy * p.Wo;
        iy0[t] = oy * p.stride - p.pad_h;
        ix0[t] = ox * p.stride - p.pad_w;
        xb[t] = p.x + (int64_t)b * p.Hi * p.Wi * ldi;
        sc[t] = EXT && p.ascale ? p.ascale + (int64_t)b * p.Cin : nullptr;
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
            a[t] = ok ? *(const f32x4*)(xb[t] + ((int64_t)iy * p.Wi + ix) * ldi + c) : f32x4{0.f, 0.f, 0.f, 0.f};
            if (EXT && ok && sc[t]) a[t] = a[t] * *(const f32x4*)(sc[t] + c);
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
                if (EXT ? p.relu == 1 : p.relu != 0) v = v > 0.f ? v : (v != v ? v : 0.f);
                if (EXT && p.relu == 2) v = v / (1.0f + expf(-v));
                if (EXT && p.res) v += p.res[(int64_t)m * p.ldr + n];
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
struct LpLayout {
    int64_t in, tap[5], pool[2], part, total;
    struct { const char* name; int64_t off, bytes; } ent[9];   // every buffer in offset order (pcdm_lpips_ws_layout)
    int n_ent;
};
inline LpLayout lpips_layout(int N, int ref_n, int H, int W, const LpGeom& g) {
    static const char* const kTap[5] = {"tap0", "tap1", "tap2", "tap3", "tap4"};
    static const char* const kPool[2] = {"pool0", "pool1"};
    const int64_t B = N + ref_n;
    LpLayout o;
    int64_t at = 0;
    const int64_t redzone = pcdm_get_workspace_redzone();   // (test hook: bytes left unused behind every buffer; 0 in product use)
    o.n_ent = 0;
    auto take = [&](const char* name, int64_t bytes) {
        const int64_t here = at;
        o.ent[o.n_ent++] = {name, here, lp_align(bytes)};
        at += lp_align(bytes) + redzone;
        return here;
    };
    o.in = take("in", B * H * W * 4 * (int64_t)sizeof(float));
    for (int l = 0; l < 5; ++l) o.tap[l] = take(kTap[l], B * g.h[l] * g.w[l] * kLpChan[l] * (int64_t)sizeof(float));
    for (int i = 0; i < 2; ++i) o.pool[i] = take(kPool[i], B * g.hp[i] * g.wp[i] * kLpChan[i] * (int64_t)sizeof(float));
    o.part = take("part", (int64_t)5 * N * kLpSlices * (int64_t)sizeof(double));
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
    ConvF32 p{x, w, bias, out + off, Hi, Wi, Cin, Ho, Wo, Cout, Npad, kh, kw, stride, pad_h, pad_w, (int)((K + 15) / 16 * 16), (int)M, relu, ldo,
              Cin, nullptr, 0, nullptr};
    PCDM_LAUNCH(conv_f32_kernel<false>, dim3((unsigned)((M + 127) / 128), (Npad + 63) / 64), dim3(256), 0, s, p);
    PCDM_CHECK_LAUNCH();
    return 0;
}
// pcdm_conv2d_f32_act: conv_f32_launch plus an input channel slice [in_off, in_off + Cin) of a tensor with ldi channels per pixel, the activation
// selector, the residual slice [res_off, res_off + Cout) of a tensor with ldr channels per pixel and the A scale
inline int conv_f32_act_launch(const float* x, int B, int Hi, int Wi, int Cin, int ldi, int in_off, const float* w, const float* bias, int Cout, int kh,
                               int kw, int stride, int pad_h, int pad_w, int act, const float* res, int ldr, int res_off, const float* ascale,
                               float* out, int ldo, int off, hipStream_t s) {
    if (!x || !w || !bias || !out || B <= 0 || Hi <= 0 || Wi <= 0 || Cin <= 0 || Cin % 4 || Cout <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || pad_h < 0 ||
        pad_w < 0 || off < 0 || ldo < Cout || off > ldo - Cout || act < 0 || act > 2)
        return -1;
    if (in_off < 0 || in_off % 4 || ldi % 4 || ldi < Cin || in_off > ldi - Cin) return -1;
    if (res && (res_off < 0 || ldr < Cout || res_off > ldr - Cout)) return -1;
    if (x == out && ldi == ldo && in_off < off + Cout && off < in_off + Cin) return -1;   // the output slice overlaps the input slice of the same tensor
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)ascale) & 15) return -1;
    if (Hi + 2 * (int64_t)pad_h < kh || Wi + 2 * (int64_t)pad_w < kw || pad_h >= 1 << 20 || pad_w >= 1 << 20) return -1;
    const int Ho = (Hi + 2 * pad_h - kh) / stride + 1, Wo = (Wi + 2 * pad_w - kw) / stride + 1;
    const int64_t M = (int64_t)B * Ho * Wo, K = (int64_t)kh * kw * Cin;
    const int Npad = (Cout + 15) / 16 * 16;
    if (M * ldo >= (int64_t)1 << 31 || (int64_t)B * Hi * Wi * ldi >= (int64_t)1 << 31 || K >= 1 << 24 || (Npad + 63) / 64 > 65535) return -1;
    if (res && M * ldr >= (int64_t)1 << 31) return -1;
    ConvF32 p{x + in_off, w, bias, out + off, Hi, Wi, Cin, Ho, Wo, Cout, Npad, kh, kw, stride, pad_h, pad_w, (int)((K + 15) / 16 * 16), (int)M, act, ldo,
              ldi, res ? res + res_off : nullptr, ldr, ascale};
    PCDM_LAUNCH(conv_f32_kernel<true>, dim3((unsigned)((M + 127) / 128), (Npad + 63) / 64), dim3(256), 0, s, p);
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

extern "C" int pcdm_conv2d_f32_ex(const float* x, int B, int Hi, int Wi, int Cin, const float* w_packed, const float* bias, int Cout, int kh, int kw,
                                  int stride, int pad_h, int pad_w, int relu, float* out, int out_pitch, int out_offset, pcdm_stream_t s) {
    return conv_f32_launch(x, B, Hi, Wi, Cin, w_packed, bias, Cout, kh, kw, stride, pad_h, pad_w, relu, out, out_pitch, out_offset, (hipStream_t)s);
}

extern "C" int pcdm_conv2d_f32_act(const float* x, int B, int Hi, int Wi, int Cin, int in_pitch, int in_offset, const float* w_packed, const float* bias,
                                   int Cout, int kh, int kw, int stride, int pad_h, int pad_w, int act, const float* residual, int res_pitch,
                                   int res_offset, const float* a_scale, float* out, int out_pitch, int out_offset, pcdm_stream_t s) {
    return conv_f32_act_launch(x, B, Hi, Wi, Cin, in_pitch, in_offset, w_packed, bias, Cout, kh, kw, stride, pad_h, pad_w, act, residual, res_pitch,
                               res_offset, a_scale, out, out_pitch, out_offset, (hipStream_t)s);
}

extern "C" int pcdm_maxpool3s2_f32_ex(const float* x, int B, int Hi, int Wi, int C, float* out, int out_pitch, int out_offset, pcdm_stream_t s) {
    return maxpool_f32_launch(x, B, Hi, Wi, C, out, out_pitch, out_offset, (hipStream_t)s);
}

extern "C" int64_t pcdm_lpips_ws_bytes(int N, int ref_n, int H, int W) {
    LpGeom g;
    if (!lpips_sizes_ok(N, ref_n, H, W) || !lpips_geom(H, W, &g)) return -1;
    return lpips_layout(N, ref_n, H, W, g).total;
}

extern "C" int pcdm_lpips_ws_layout(int N, int ref_n, int H, int W, int index, const char** name, int64_t* offset, int64_t* bytes) {
    LpGeom g;
    if (!lpips_sizes_ok(N, ref_n, H, W) || !lpips_geom(H, W, &g)) return -1;
    const LpLayout lay = lpips_layout(N, ref_n, H, W, g);
    if (index == -1) return lay.n_ent;
    if (index < 0 || index >= lay.n_ent) return -1;
    if (name) *name = lay.ent[index].name;
    if (offset) *offset = lay.ent[index].off;
    if (bytes) *bytes = lay.ent[index].bytes;
    return lay.n_ent;
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
struct IncLayout { int64_t at[kIncBufs], bytes[kIncBufs], total; };
inline IncLayout inception_layout(int B, const IncPlan& p) {
    IncLayout o;
    int64_t at = 0;
    const int64_t redzone = pcdm_get_workspace_redzone();   // (test hook: bytes left unused behind every buffer; 0 in product use)
    for (int i = 0; i < kIncBufs; ++i) {
        o.at[i] = at;
        o.bytes[i] = lp_align((int64_t)B * p.elems[i] * (int64_t)sizeof(float));
        at += o.bytes[i] + redzone;
    }
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

extern "C" int pcdm_inception_ws_layout(int B, int H, int W, int dims, int index, const char** name, int64_t* offset, int64_t* bytes) {
    static const char* const kNames[kIncBufs] = {"x", "a", "b", "t", "u", "p"};   // enum order: the input, the ping-pong pair, a block's three intermediates
    IncPlan p;
    if (!inception_sizes_ok(B, H, W) || !inception_plan(H, W, dims, &p)) return -1;
    if (index == -1) return kIncBufs;
    if (index < 0 || index >= kIncBufs) return -1;
    const IncLayout lay = inception_layout(B, p);
    if (name) *name = kNames[index];
    if (offset) *offset = lay.at[index];
    if (bytes) *bytes = lay.bytes[index];
    return kIncBufs;
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
