#include "pcdm_device.h"
#include "../../include/pcdm.h"
#include "image_common.h"

// ---- DWPose pose maps from keypoints (controlnet_aux dwpose: DWposeDetector.__call__ after the networks -> draw_pose -> draw_bodypose /
// draw_handpose / draw_facepose, then cv2.resize(..., INTER_LINEAR)) ---------------------------------------------------------------------------
// Two passes.  The primitive pass repeats the reference's arithmetic from keypoints to integers (fp32, the limb angle in double, every operation
// its own IEEE operation) and fills a fixed-slot table of integer primitives in the reference's draw order; the raster pass decides coverage in
// integers only (include/pcdm.h states the rules), so the bytes depend on nothing but the table.  No atomics; no launch-order dependence: a pixel
// takes the LAST primitive of the table that covers it, which is what drawing them one after another leaves behind.
namespace {
constexpr int kPdSlots = 185;                   // per person: 17 limbs + 18 joints + 2 hands x (20 edges + 21 points) + 68 face points
constexpr int kPdInts = 8;                      // int32 per slot: {kind, p0, p1, p2, p3, p4, colour, 0}
constexpr int kPdMaxPersons = 32, kPdMaxSide = 4096;
constexpr int kPdTW = 32, kPdTH = 8;            // pixel tile of pose_raster_kernel: one pixel per lane
constexpr int kPdTableInts = 360 * 2 + 20;      // pcdm_pose_tables: {C, S} of every whole degree, then the 20 hand-edge colours
enum { PD_EMPTY = 0, PD_LIMB = 1, PD_DISC = 2, PD_LINE = 3 };
//   PD_LIMB: {cx, cy, a, C, S}   PD_DISC: {x, y, r}   PD_LINE: {x0, y0, x1, y1}

__device__ __forceinline__ uint32_t pd_rgb(int r, int g, int b) { return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16); }

// int(math.degrees(math.atan2(y, x))): the multiples of 45 degrees are exact by case, so that a last-bit difference between two atan2
// implementations cannot move a truncation across a whole degree; between them no fp32 pair comes that close to one
__device__ __forceinline__ int pd_angle(float yf, float xf) {
    const double y = (double)yf, x = (double)xf;
    if (!(y == y) || !(x == x)) return 0;
    const double ay = fabs(y), ax = fabs(x);
    const bool yneg = __builtin_signbit(y), xneg = __builtin_signbit(x);
    if (ay == 0.0) return xneg ? (yneg ? -180 : 180) : 0;
    if (ax == 0.0) return yneg ? -90 : 90;
    if (ay == ax) return (yneg ? -1 : 1) * (xneg ? 135 : 45);
    return (int)(atan2(y, x) * (180.0 / 3.14159265358979323846));
}

struct PdSlot { int kind, p0, p1, p2, p3, p4; uint32_t colour; };

// Slot `s` of one map with P persons, in draw order: limbs (for i: for person), joints (for i: for person), all left hands then all right hands
// (20 edges, then 21 points each), face points.  kp [P, 134, 2], sc [P, 134] of that map.
__device__ __forceinline__ PdSlot pd_slot(const float* __restrict__ kp, const float* __restrict__ sc, int P, int s, int H, int W, int hands, int faces,
                                          const int32_t* __restrict__ tables) {
#pragma clang fp contract(off)
    static constexpr int kLimb[17][2] = {{1, 2}, {1, 5}, {2, 3}, {3, 4}, {5, 6}, {6, 7}, {1, 8}, {8, 9}, {9, 10}, {1, 11}, {11, 12}, {12, 13}, {1, 0}, {0, 14},
                              {14, 16}, {0, 15}, {15, 17}};
    static constexpr int kBody[18][3] = {{255, 0, 0}, {255, 85, 0}, {255, 170, 0}, {255, 255, 0}, {170, 255, 0}, {85, 255, 0}, {0, 255, 0}, {0, 255, 85},
                              {0, 255, 170}, {0, 255, 255}, {0, 170, 255}, {0, 85, 255}, {0, 0, 255}, {85, 0, 255}, {170, 0, 255}, {255, 0, 255},
                              {255, 0, 170}, {255, 0, 85}};
    static constexpr int kEdge[20][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {0, 5}, {5, 6}, {6, 7}, {7, 8}, {0, 9}, {9, 10}, {10, 11}, {11, 12}, {0, 13}, {13, 14},
                              {14, 15}, {15, 16}, {0, 17}, {17, 18}, {18, 19}, {19, 20}};
    PdSlot o{PD_EMPTY, 0, 0, 0, 0, 0, 0u};
    const float Wf = (float)W, Hf = (float)H;
    // candidate[..., 0] /= float(W); candidate[..., 1] /= float(H): one fp32 division each
    auto cx = [&](int n, int j) { return kp[((int64_t)n * 134 + j) * 2] / Wf; };
    auto cy = [&](int n, int j) { return kp[((int64_t)n * 134 + j) * 2 + 1] / Hf; };
    if (s < 17 * P) {                                             // ---- limb: an ellipse of half-axes (int(length / 2), 4)
        const int i = s / P, n = s - i * P, j0 = kLimb[i][0], j1 = kLimb[i][1];
        if (!(sc[n * 134 + j0] > 0.3f) || !(sc[n * 134 + j1] > 0.3f)) return o;
        const float Y0 = cv_mul(cx(n, j0), Wf), Y1 = cv_mul(cx(n, j1), Wf);          // Y = candidate[index, 0] * float(W)
        const float X0 = cv_mul(cy(n, j0), Hf), X1 = cv_mul(cy(n, j1), Hf);          // X = candidate[index, 1] * float(H)
        const float mX = (X0 + X1) / 2.0f, mY = (Y0 + Y1) / 2.0f;
        const float dX = X0 - X1, dY = Y0 - Y1;
        const float len = sqrtf(cv_mul(dX, dX) + cv_mul(dY, dY));
        const int a = cv_trunc(len / 2.0f);
        if (a < 0) return o;                                      // (a NaN coordinate)
        int th = pd_angle(dX, dY) % 360;
        if (th < 0) th += 360;
        o = PdSlot{PD_LIMB, cv_trunc(mY), cv_trunc(mX), a, tables[2 * th], tables[2 * th + 1], pd_rgb(kBody[i][0], kBody[i][1], kBody[i][2])};
        return o;
    }
    s -= 17 * P;
    if (s < 18 * P) {                                             // ---- body joint: a disc of radius 4, no coordinate test
        const int i = s / P, n = s - i * P;
        if (!(sc[n * 134 + i] > 0.3f)) return o;
        o = PdSlot{PD_DISC, cv_trunc(cv_mul(cx(n, i), Wf)), cv_trunc(cv_mul(cy(n, i), Hf)), 4, 0, 0, pd_rgb(kBody[i][0], kBody[i][1], kBody[i][2])};
        return o;
    }
    s -= 18 * P;
    // a hand or face point whose score is below 0.3 becomes (-1, -1) before it is scaled: int(-1 * W) fails the x > eps test
    auto px = [&](int n, int j) { return cv_trunc(cv_mul(sc[n * 134 + j] < 0.3f ? -1.0f : cx(n, j), Wf)); };
    auto py = [&](int n, int j) { return cv_trunc(cv_mul(sc[n * 134 + j] < 0.3f ? -1.0f : cy(n, j), Hf)); };
    if (s < 82 * P) {                                             // ---- hands
        if (!hands) return o;
        const int h = s / 41, e = s - h * 41;                     // h: the left hands of every person, then the right hands
        const int n = h < P ? h : h - P, base = h < P ? 92 : 113;
        if (e < 20) {
            const int j0 = base + kEdge[e][0], j1 = base + kEdge[e][1];
            const int x1 = px(n, j0), y1 = py(n, j0), x2 = px(n, j1), y2 = py(n, j1);
            if (x1 < 1 || y1 < 1 || x2 < 1 || y2 < 1) return o;
            o = PdSlot{PD_LINE, x1, y1, x2, y2, 0, (uint32_t)tables[720 + e] & 0xffffffu};
        } else {
            const int x = px(n, base + e - 20), y = py(n, base + e - 20);
            if (x < 1 || y < 1) return o;
            o = PdSlot{PD_DISC, x, y, 1, 0, 0, pd_rgb(0, 0, 255)};
        }
        return o;
    }
    s -= 82 * P;
    if (!faces) return o;                                         // ---- face points
    const int n = s / 68, j = 24 + s - n * 68;
    const int x = px(n, j), y = py(n, j);
    if (x < 1 || y < 1) return o;
    o = PdSlot{PD_DISC, x, y, 3, 0, 0, pd_rgb(255, 255, 255)};
    return o;
}

// prims [M, P * 185, 8] int32 <- keypoints [M, P, 134, 2], scores [M, P, 134]; one slot per lane
__global__ __launch_bounds__(256) void pose_prims_kernel(const float* __restrict__ kp, const float* __restrict__ sc, int M, int P, int H, int W, int hands,
                                                         int faces, const int32_t* __restrict__ tables, int32_t* __restrict__ prims) {
    const int n = P * kPdSlots;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * n) return;
    const int m = i / n, s = i - m * n;
    const PdSlot o = pd_slot(kp + (int64_t)m * P * 134 * 2, sc + (int64_t)m * P * 134, P, s, H, W, hands, faces, tables);
    int32_t* d = prims + (int64_t)i * kPdInts;
    d[0] = o.kind; d[1] = o.p0; d[2] = o.p1; d[3] = o.p2; d[4] = o.p3; d[5] = o.p4; d[6] = (int32_t)o.colour; d[7] = 0;
}

// may primitive p touch the pixel rectangle [x0, x1] x [y0, y1]?  Conservative: the exact rule is pd_covers
__device__ __forceinline__ bool pd_touches(const int32_t* __restrict__ p, int x0, int y0, int x1, int y1) {
    int lx, ly, hx, hy;
    switch (p[0]) {
    case PD_LIMB: {               // inside the circle of radius max(a, 4) + 1/2 about the centre; (a >> 13): the rounding of C and S to 2^-14
        const int R = imax(p[3], 4) + 2 + (p[3] >> 13);
        lx = p[1] - R; hx = p[1] + R; ly = p[2] - R; hy = p[2] + R;
        break;
    }
    case PD_DISC:
        lx = p[1] - p[3]; hx = p[1] + p[3]; ly = p[2] - p[3]; hy = p[2] + p[3];
        break;
    case PD_LINE:
        lx = imin(p[1], p[3]); hx = imax(p[1], p[3]); ly = imin(p[2], p[4]); hy = imax(p[2], p[4]);
        break;
    default:
        return false;
    }
    return hx >= x0 && lx <= x1 && hy >= y0 && ly <= y1;
}

__device__ __forceinline__ int64_t pd_abs64(int64_t v) { return v < 0 ? -v : v; }

// the coverage rules of include/pcdm.h, integers only
__device__ __forceinline__ bool pd_covers(const int32_t* __restrict__ p, int x, int y) {
    switch (p[0]) {
    case PD_LIMB: {
        const int64_t dx = (int64_t)x - p[1], dy = (int64_t)y - p[2], C = p[4], S = p[5];
        const int64_t u = 2 * (dx * C + dy * S), v = 2 * (dy * C - dx * S);
        const int64_t A = 2 * (int64_t)p[3] + 1, B = 9;
        if (pd_abs64(u) > A * 16384 || pd_abs64(v) > B * 16384) return false;
        // below 2^63 while A < 2^13.8, which every limb with both ends on a canvas of 4096 has; a keypoint far outside the frame can exceed it,
        // so the sum is taken in 128 bits
        typedef unsigned __int128 u128;
        const uint64_t au = (uint64_t)pd_abs64(u), av = (uint64_t)pd_abs64(v), AA = (uint64_t)(A * A), BB = (uint64_t)(B * B);
        return (u128)BB * ((u128)au * au) + (u128)AA * ((u128)av * av) <= ((u128)AA * BB) << 28;
    }
    case PD_DISC: {
        const int64_t dx = (int64_t)x - p[1], dy = (int64_t)y - p[2], r = p[3];
        return dx * dx + dy * dy <= r * r + r / 2;
    }
    case PD_LINE: {               // the pixel of step k along the major axis, evaluated for this pixel's k
        const int64_t ddx = (int64_t)p[3] - p[1], ddy = (int64_t)p[4] - p[2];
        const int64_t adx = pd_abs64(ddx), ady = pd_abs64(ddy);
        const bool xmajor = adx >= ady;
        const int64_t dmaj = xmajor ? ddx : ddy, dmin = xmajor ? ddy : ddx, amaj = xmajor ? adx : ady, amin = xmajor ? ady : adx;
        const int64_t qmaj = xmajor ? (int64_t)x - p[1] : (int64_t)y - p[2], qmin = xmajor ? (int64_t)y - p[2] : (int64_t)x - p[1];
        if (amaj == 0) return qmaj == 0 && qmin == 0;
        const int64_t k = dmaj < 0 ? -qmaj : qmaj;
        if (k < 0 || k > amaj) return false;
        const int64_t step = (2 * k * amin + amaj) / (2 * amaj);
        return qmin == (dmin < 0 ? -step : step);
    }
    default:
        return false;
    }
}

// One workgroup per 32 x 8 pixel tile of map blockIdx.z.  Lane t tests the slots [t K, (t + 1) K) of the map's table against the tile; the counts
// are prefix-summed through LDS and the surviving slot numbers written in table order.  Then every pixel walks the survivors from the last to the
// first and takes the first that covers it: a limb at colour * 3 / 5 (the canvas * 0.6 the reference applies after the limb layer), anything
// else as is; a pixel nothing covers is black, so the canvas needs no clearing.
__global__ __launch_bounds__(256) void pose_raster_kernel(const int32_t* __restrict__ prims, int n, uint8_t* __restrict__ out, int H, int W) {
    __shared__ uint16_t list[kPdMaxPersons * kPdSlots];
    __shared__ int count[256];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kPdTW, y0 = blockIdx.y * kPdTH;
    const int x1 = imin(x0 + kPdTW, W) - 1, y1 = imin(y0 + kPdTH, H) - 1;
    const int32_t* mp = prims + (int64_t)blockIdx.z * n * kPdInts;
    const int K = (n + 255) / 256, lo = imin(tid * K, n), hi = imin(lo + K, n);
    int c = 0;
    for (int s = lo; s < hi; ++s) c += pd_touches(mp + (int64_t)s * kPdInts, x0, y0, x1, y1) ? 1 : 0;
    count[tid] = c;
    __syncthreads();
    int off = 0, total = 0;
    for (int t = 0; t < 256; ++t) {
        const int v = count[t];
        off += t < tid ? v : 0;
        total += v;
    }
    for (int s = lo; s < hi; ++s)
        if (pd_touches(mp + (int64_t)s * kPdInts, x0, y0, x1, y1)) list[off++] = (uint16_t)s;
    __syncthreads();
    const int x = x0 + (tid & (kPdTW - 1)), y = y0 + tid / kPdTW;
    if (x >= W || y >= H) return;
    uint32_t rgb = 0;
    for (int i = total - 1; i >= 0; --i) {
        const int32_t* p = mp + (int64_t)list[i] * kPdInts;
        if (!pd_covers(p, x, y)) continue;
        rgb = (uint32_t)p[6];
        if (p[0] == PD_LIMB) rgb = pd_rgb((int)(rgb & 255u) * 3 / 5, (int)((rgb >> 8) & 255u) * 3 / 5, (int)((rgb >> 16) & 255u) * 3 / 5);
        break;
    }
    uint8_t* d = out + (((int64_t)blockIdx.z * H + y) * W + x) * 3;
    d[0] = (uint8_t)rgb;
    d[1] = (uint8_t)(rgb >> 8);
    d[2] = (uint8_t)(rgb >> 16);
}

// ---- cv2.resize(uint8 image, INTER_LINEAR) in OpenCV's 8-bit fixed-point form (include/pcdm.h) -----------------------------------------------
// dst [M, Hd, Wd, 3] <- src [M, Hs, Ws, 3]; one output pixel per lane
__global__ __launch_bounds__(256) void resize_linear_kernel(const uint8_t* __restrict__ src, int M, int Hs, int Ws, double scale_x, double scale_y,
                                                            uint8_t* __restrict__ dst, int Hd, int Wd) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)M * Hd * Wd) return;
    const int x = (int)(i % Wd), y = (int)((i / Wd) % Hd), m = (int)(i / ((int64_t)Wd * Hd));
    int xa, xb, a0, a1, ya, yb, b0, b1;
    cv_lin_coeff(x, scale_x, Ws, true, xa, xb, a0, a1);
    cv_lin_coeff(y, scale_y, Hs, false, ya, yb, b0, b1);
    const uint8_t* r0 = src + ((int64_t)m * Hs + ya) * Ws * 3;
    const uint8_t* r1 = src + ((int64_t)m * Hs + yb) * Ws * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int S0 = (int)r0[xa * 3 + c] * a0 + (int)r0[xb * 3 + c] * a1;
        const int S1 = (int)r1[xa * 3 + c] * a0 + (int)r1[xb * 3 + c] * a1;
        const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
        dst[i * 3 + c] = (uint8_t)imin(imax(v, 0), 255);
    }
}

bool pd_sizes_ok(int M, int P, int H, int W) {
    return M >= 0 && M <= 65535 && P >= 0 && P <= kPdMaxPersons && H > 0 && W > 0 && H <= kPdMaxSide && W <= kPdMaxSide;
}
}  // namespace

extern "C" int pcdm_pose_tables(int32_t* tables, int count) {
    if (!tables || count != kPdTableInts) return -1;
    const double pi = 3.14159265358979323846;
    for (int t = 0; t < 360; ++t) {
        tables[2 * t] = (int32_t)lround(cos((double)t * pi / 180.0) * 16384.0);
        tables[2 * t + 1] = (int32_t)lround(sin((double)t * pi / 180.0) * 16384.0);
    }
    for (int e = 0; e < 20; ++e) {            // matplotlib.colors.hsv_to_rgb([e / 20, 1, 1]) * 255, rounded half to even
        const double h = (double)e / 20.0, s = 1.0, v = 1.0;
        const int i = (int)(h * 6.0);
        const double f = h * 6.0 - (double)i;
        const double p = v * (1.0 - s), q = v * (1.0 - s * f), t = v * (1.0 - s * (1.0 - f));
        double r, g, b;
        switch (i % 6) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
        }
        tables[720 + e] = (int32_t)((uint32_t)nearbyint(r * 255.0) | ((uint32_t)nearbyint(g * 255.0) << 8) | ((uint32_t)nearbyint(b * 255.0) << 16));
    }
    return 0;
}

extern "C" int64_t pcdm_pose_ws_bytes(int M, int P) {
    if (!pd_sizes_ok(M, P, 1, 1)) return -1;
    return (int64_t)M * P * kPdSlots * kPdInts * (int64_t)sizeof(int32_t);
}

extern "C" int pcdm_pose_draw(const float* keypoints, const float* scores, int M, int P, int Hd, int Wd, int hands, int faces, const int32_t* tables,
                              void* out, void* ws, int64_t ws_bytes, pcdm_stream_t s) {
    if (!pd_sizes_ok(M, P, Hd, Wd) || !out || !tables) return -1;
    if (M == 0) return 0;
    const int n = P * kPdSlots;
    if (n > 0) {
        if (!keypoints || !scores || !ws || ((uintptr_t)ws & 3) || ws_bytes < pcdm_pose_ws_bytes(M, P)) return -1;
        PCDM_LAUNCH(pose_prims_kernel, grid1d((int64_t)M * n, 256), dim3(256), 0, (hipStream_t)s, keypoints, scores, M, P, Hd, Wd, hands != 0, faces != 0,
                    tables, (int32_t*)ws);
        PCDM_CHECK_LAUNCH();
    }
    PCDM_LAUNCH(pose_raster_kernel, dim3((Wd + kPdTW - 1) / kPdTW, (Hd + kPdTH - 1) / kPdTH, M), dim3(256), 0, (hipStream_t)s, (const int32_t*)ws, n,
                (uint8_t*)out, Hd, Wd);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_resize_linear_u8(const void* src, int M, int Hs, int Ws, void* dst, int Hd, int Wd, pcdm_stream_t s) {
    if (!src || !dst || M < 0 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0) return -1;
    if ((int64_t)M * Hs * Ws * 3 >= (int64_t)1 << 31 || (int64_t)M * Hd * Wd * 3 >= (int64_t)1 << 31) return -1;
    if (M == 0) return 0;
    const double scale_x = 1.0 / ((double)Wd / (double)Ws), scale_y = 1.0 / ((double)Hd / (double)Hs);
    PCDM_LAUNCH(resize_linear_kernel, grid1d((int64_t)M * Hd * Wd, 256), dim3(256), 0, (hipStream_t)s, (const uint8_t*)src, M, Hs, Ws, scale_x, scale_y,
                (uint8_t*)dst, Hd, Wd);
    PCDM_CHECK_LAUNCH();
    return 0;
}
