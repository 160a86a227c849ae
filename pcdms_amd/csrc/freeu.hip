// FreeU (arXiv 2309.11497; diffusers 0.24.0 apply_freeu / fourier_filter) for one decoder resnet, in front of its [hidden | skip] concat:
//     hidden[:, : C1 / 2] *= b                      (first half of the backbone channels)
//     skip = ifftn(ifftshift(fftshift(fftn(skip)) * mask)).real over (H, W), mask = 1 except s on the centred 2 x 2 block (threshold 1)
// The 2 x 2 block holds the frequencies ky in {0, -1}, kx in {0, -1} (one frequency along an axis of length 1; -1 is the Nyquist frequency at
// length 2), so the filter is a projection onto at most four DFT coefficients per (image, channel) plane -- no FFT:
//     skip' = skip + (s - 1) / (H W) * [ S + (Ac cy + As sy) + (Bc cx + Bs sx) + (Dc cxy + Ds sxy) ]
// with cy + i sy = e^{2 pi i y / H}, cx + i sx = e^{2 pi i x / W}, cxy + i sxy their product, and the seven plane sums S = sum v, Ac = sum v cy, ...
// (the real part needs no separate +1 frequencies: they are the conjugates).
//
// Precision: the plane sums and the correction are carried in fp64 and the result is rounded to bf16 once.  fp32 sums are NOT enough for a
// one-ulp result: at s = 0.2 the correction cancels single elements to |skip'| ~ 1e-4, where one bf16 ulp is 5e-7 -- the size of the error of an
// fp32 sum over 352 pixels (measured: 3 ulp).  The work is a few MFLOP per launch; the launch, not the arithmetic, is what it costs.
//
// Tensors are the UNet schedule's: bf16 NHWC rows, hidden [B HW, C1], skip [B HW, C2].  ONE launch per resnet: a workgroup owns the slab of
// (image, 64 channels = one 128-byte line per pixel) with all its pixels in LDS between the reduction and the apply; the same grid scales the
// backbone.  Planes whose slab does not fit (HW > kOneLaunchPixels) take two launches: coefficients into a workspace, then the apply.  The
// plane sums are added in a fixed order (four interleaved pixel partitions, then the partitions in order), the same in both forms: no atomics,
// reruns are bit-identical, and a plane's result does not depend on its place in the batch.
#include "pcdm_device.h"
#include "../../include/pcdm.h"

namespace {
constexpr int kThreads = 256;
constexpr int kChunk = 64;     // channels per workgroup: 128 bytes of every pixel row
constexpr int kParts = kThreads / kChunk;   // pixel partitions of the reduction
constexpr int kCoef = 7;
constexpr int kLdsBudget = 64 * 1024;       // dynamic LDS a launch gets without an opt-in attribute
constexpr int kLdsFixed = kParts * kCoef * kChunk * 8 + 16;    // the partitions' sums (fp64) + the odd entry of the twiddle tables (H + W <= HW + 1)
constexpr int kLdsPerPixel = kChunk * 2 + 16;                  // the slab row + one {cos, sin} fp64 pair of the row / column tables
constexpr int kOneLaunchPixels = (kLdsBudget - kLdsFixed) / kLdsPerPixel;   // = 355: 8 x 11 and 16 x 22 fit
constexpr int kTile = 32;      // pixels per workgroup of the two-launch apply

struct Tw { double cy, sy, cx, sx; };
struct Cs { double c, s; };

// e^{2 pi i k / n}
__device__ __forceinline__ Cs unit_root(int k, int n) {
    Cs r;
#ifdef PCDM_EMU
    const double a = 6.283185307179586476925 * (double)k / (double)n;
    r.c = cos(a);
    r.s = sin(a);
#else
    sincospi(2.0 * (double)k / (double)n, &r.s, &r.c);
#endif
    return r;
}
__device__ __forceinline__ Tw pixel_twiddles(int p, int H, int W) {   // of pixel p = y W + x
    const Cs y = unit_root(p / W, H), x = unit_root(p % W, W);
    return Tw{y.c, y.s, x.c, x.s};
}
__device__ __forceinline__ void accumulate(double* a, float vf, const Tw& t) {
    const double v = (double)vf;
    const double cxy = t.cy * t.cx - t.sy * t.sx, sxy = t.sy * t.cx + t.cy * t.sx;
    a[0] += v;
    a[1] += v * t.cy;
    a[2] += v * t.sy;
    a[3] += v * t.cx;
    a[4] += v * t.sx;
    a[5] += v * cxy;
    a[6] += v * sxy;
}
// the partitions' sums -> one of the plane's seven coefficients (fixed order); the frequency sets are deduplicated along an axis of length 1
__device__ __forceinline__ double combine(const double* part, int k, int c, int H, int W) {
    double v = part[(0 * kCoef + k) * kChunk + c];
#pragma unroll
    for (int q = 1; q < kParts; ++q) v += part[(q * kCoef + k) * kChunk + c];
    const bool drop = ((k == 1 || k == 2 || k >= 5) && H == 1) || (k >= 3 && W == 1);
    return drop ? 0.0 : v;
}
// eight channels of one pixel: coef[k][e] (k < 7, e < 8), g = (s - 1) / (H W)
__device__ __forceinline__ u32x4 apply8(u32x4 raw, const double (*coef)[8], const Tw& t, double g) {
    if (g == 0.0) return raw;   // (s = 1: the identity, bit for bit)
    const double cxy = t.cy * t.cx - t.sy * t.sx, sxy = t.sy * t.cx + t.cy * t.sx;
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float r[2];
#pragma unroll
        for (int hl = 0; hl < 2; ++hl) {
            const int ch = 2 * e + hl;
            const double v = (double)bf2f((u16)(hl ? raw[e] >> 16 : raw[e] & 0xffffu));
            const double R = coef[0][ch] + (coef[1][ch] * t.cy + coef[2][ch] * t.sy) + (coef[3][ch] * t.cx + coef[4][ch] * t.sx) +
                             (coef[5][ch] * cxy + coef[6][ch] * sxy);
            r[hl] = (float)(v + g * R);
        }
        o[e] = pack2bf(r[0], r[1]);
    }
    return o;
}
// the backbone of image b in units of four channels (C1 % 8 == 0: the half is a multiple of 4): out = bf16(float(x) * b) on the first half, the
// second half copied unless in place.  `part` of `nparts` workgroups share the image.
__device__ __forceinline__ void scale_backbone(const u16* __restrict__ hin, u16* __restrict__ hout, int64_t row0, int HW, int C1, float b, int part, int nparts) {
    const int upr = C1 / 4, half = C1 / 8;   // units per row, units of the scaled half
    const bool inplace = hin == hout;
    const int64_t total = (int64_t)HW * upr;
    for (int64_t u = (int64_t)part * kThreads + threadIdx.x; u < total; u += (int64_t)nparts * kThreads) {
        const int cu = (int)(u % upr);
        if (cu >= half && inplace) continue;
        const int64_t off = (row0 + u / upr) * C1 + (int64_t)cu * 4;
        u32x2 v = *(const u32x2*)(hin + off);
        if (cu < half) {
            v[0] = pack2bf(bf2f((u16)(v[0] & 0xffffu)) * b, bf2f((u16)(v[0] >> 16)) * b);
            v[1] = pack2bf(bf2f((u16)(v[1] & 0xffffu)) * b, bf2f((u16)(v[1] >> 16)) * b);
        }
        *(u32x2*)(hout + off) = v;
    }
}

// ---- one launch: grid (channel chunks of the skip, B)
__global__ __launch_bounds__(kThreads) void freeu_slab_kernel(const u16* __restrict__ hin, u16* __restrict__ hout, const u16* __restrict__ skip,
                                                              u16* __restrict__ sout, int H, int W, int C1, int C2, float b, double g) {
    PCDM_DYN_SMEM(smem);
    const int HW = H * W, t = threadIdx.x;
    const int c0 = blockIdx.x * kChunk;
    const int64_t row0 = (int64_t)blockIdx.y * HW;
    double* part = (double*)smem;                                // [kParts][7][64]
    Cs* twy = (Cs*)(part + kParts * kCoef * kChunk);             // [H]
    Cs* twx = twy + H;                                           // [W]
    u16* slab = (u16*)(twx + W);                                 // [HW][64]
    for (int i = t; i < H + W; i += kThreads) twy[i] = i < H ? unit_root(i, H) : unit_root(i - H, W);
    const int cv = t & 7, pl = t >> 3;                           // eight lanes = one 128-byte pixel row of the chunk
    const bool cv_ok = c0 + cv * 8 < C2;                         // (C2 % 8 == 0: a vector of eight channels is inside or outside as a whole)
    for (int p = pl; p < HW; p += kThreads / 8) {
        u32x4 v = {0, 0, 0, 0};
        if (cv_ok) v = *(const u32x4*)(skip + (row0 + p) * C2 + c0 + cv * 8);
        *(u32x4*)(slab + p * kChunk + cv * 8) = v;
    }
    __syncthreads();
    {   // plane sums: thread = (channel, pixel partition)
        const int c = t & (kChunk - 1), q = t / kChunk;
        double a[kCoef] = {0., 0., 0., 0., 0., 0., 0.};
        for (int p = q; p < HW; p += kParts) {
            const Cs y = twy[p / W], x = twx[p % W];
            accumulate(a, bf2f(slab[p * kChunk + c]), Tw{y.c, y.s, x.c, x.s});
        }
#pragma unroll
        for (int k = 0; k < kCoef; ++k) part[(q * kCoef + k) * kChunk + c] = a[k];
    }
    __syncthreads();
    if (cv_ok) {
        double coef[kCoef][8];
#pragma unroll
        for (int k = 0; k < kCoef; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) coef[k][e] = combine(part, k, cv * 8 + e, H, W);
        for (int p = pl; p < HW; p += kThreads / 8) {
            const Cs y = twy[p / W], x = twx[p % W];
            *(u32x4*)(sout + (row0 + p) * C2 + c0 + cv * 8) = apply8(*(const u32x4*)(slab + p * kChunk + cv * 8), coef, Tw{y.c, y.s, x.c, x.s}, g);
        }
    }
    scale_backbone(hin, hout, row0, HW, C1, b, blockIdx.x, gridDim.x);
}

// ---- two launches, any plane size.  (1) the coefficients of every (image, channel): grid (channel chunks, B) -> ws fp64 [B][7][C2]
__global__ __launch_bounds__(kThreads) void freeu_coef_kernel(const u16* __restrict__ skip, double* __restrict__ ws, int H, int W, int C2) {
    __shared__ Tw tw[kThreads];
    __shared__ double part[kParts * kCoef * kChunk];
    const int HW = H * W, t = threadIdx.x;
    const int c = t & (kChunk - 1), q = t / kChunk, ch = blockIdx.x * kChunk + c;
    const int64_t row0 = (int64_t)blockIdx.y * HW;
    double a[kCoef] = {0., 0., 0., 0., 0., 0., 0.};
    for (int p0 = 0; p0 < HW; p0 += kThreads) {   // (kThreads % kParts == 0: the partitions see their pixels in the one-launch order)
        __syncthreads();
        if (p0 + t < HW) tw[t] = pixel_twiddles(p0 + t, H, W);
        __syncthreads();
        const int n = HW - p0 < kThreads ? HW - p0 : kThreads;
        if (ch < C2)
            for (int i = q; i < n; i += kParts) accumulate(a, bf2f(skip[(row0 + p0 + i) * C2 + ch]), tw[i]);
    }
#pragma unroll
    for (int k = 0; k < kCoef; ++k) part[(q * kCoef + k) * kChunk + c] = a[k];
    __syncthreads();
    for (int i = t; i < kCoef * kChunk; i += kThreads) {
        const int k = i / kChunk, cc = blockIdx.x * kChunk + i % kChunk;
        if (cc < C2) ws[((int64_t)blockIdx.y * kCoef + k) * C2 + cc] = combine(part, k, i % kChunk, H, W);
    }
}
// (2) the apply and the backbone: grid (tiles of kTile pixels, B)
__global__ __launch_bounds__(kThreads) void freeu_apply_kernel(const u16* __restrict__ hin, u16* __restrict__ hout, const u16* __restrict__ skip,
                                                               u16* __restrict__ sout, const double* __restrict__ ws, int H, int W, int C1, int C2,
                                                               float b, double g) {
    __shared__ Tw tw[kTile];
    const int HW = H * W, t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.y * HW;
    const int p0 = blockIdx.x * kTile;
    if (t < kTile && p0 + t < HW) tw[t] = pixel_twiddles(p0 + t, H, W);
    __syncthreads();
    const int cv = t & 7, pl = t >> 3, p = p0 + pl;
    if (p < HW) {
        const double* cf = ws + (int64_t)blockIdx.y * kCoef * C2;
        for (int c = cv * 8; c < C2; c += 64) {
            double coef[kCoef][8];
#pragma unroll
            for (int k = 0; k < kCoef; ++k)
#pragma unroll
                for (int e = 0; e < 8; ++e) coef[k][e] = cf[(int64_t)k * C2 + c + e];
            const int64_t off = (row0 + p) * C2 + c;
            *(u32x4*)(sout + off) = apply8(*(const u32x4*)(skip + off), coef, tw[pl], g);
        }
    }
    scale_backbone(hin, hout, row0, HW, C1, b, blockIdx.x, gridDim.x);
}

bool freeu_shape_ok(int B, int H, int W, int C1, int C2) {
    return B >= 1 && H >= 1 && W >= 1 && C1 >= 8 && C2 >= 8 && C1 % 8 == 0 && C2 % 8 == 0 && (int64_t)H * W <= (1 << 24) && B <= 65535 &&
           (int64_t)B * H * W * (C1 > C2 ? C1 : C2) < ((int64_t)1 << 40);
}
}  // namespace

extern "C" int64_t pcdm_freeu_ws_bytes(int B, int H, int W, int C1, int C2) {
    if (!freeu_shape_ok(B, H, W, C1, C2)) return -1;
    if ((int64_t)H * W <= kOneLaunchPixels) return 0;
    return ((int64_t)B * kCoef * C2 * 8 + 255) / 256 * 256;
}

extern "C" int pcdm_freeu(const void* hidden, void* hidden_out, const void* skip, void* skip_out, int B, int H, int W, int C1, int C2, float b, float s,
                          void* workspace, pcdm_stream_t st) {
    if (!hidden || !hidden_out || !skip || !skip_out || skip == skip_out || !freeu_shape_ok(B, H, W, C1, C2)) return -1;
    if ((((uintptr_t)hidden | (uintptr_t)hidden_out | (uintptr_t)skip | (uintptr_t)skip_out) & 15)) return -1;
    const int HW = H * W, chunks = (C2 + kChunk - 1) / kChunk;
    const double g = ((double)s - 1.0) / (double)HW;
    if (HW <= kOneLaunchPixels) {
        const size_t lds = (size_t)kParts * kCoef * kChunk * 8 + (size_t)(H + W) * 16 + (size_t)HW * kChunk * 2;   // <= kLdsBudget: H + W <= HW + 1
        PCDM_LAUNCH(freeu_slab_kernel, dim3(chunks, B), dim3(kThreads), lds, (hipStream_t)st, (const u16*)hidden, (u16*)hidden_out, (const u16*)skip,
                    (u16*)skip_out, H, W, C1, C2, b, g);
        PCDM_CHECK_LAUNCH();
        return 0;
    }
    if (!workspace || ((uintptr_t)workspace & 15)) return -1;
    PCDM_LAUNCH(freeu_coef_kernel, dim3(chunks, B), dim3(kThreads), 0, (hipStream_t)st, (const u16*)skip, (double*)workspace, H, W, C2);
    PCDM_CHECK_LAUNCH();
    PCDM_LAUNCH(freeu_apply_kernel, dim3((HW + kTile - 1) / kTile, B), dim3(kThreads), 0, (hipStream_t)st, (const u16*)hidden, (u16*)hidden_out,
                (const u16*)skip, (u16*)skip_out, (const double*)workspace, H, W, C1, C2, b, g);
    PCDM_CHECK_LAUNCH();
    return 0;
}
