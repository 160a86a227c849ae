#include "pcdm_device.h"
#include "../../include/pcdm.h"
#include "image_common.h"

// ---- The person detector (mmdet's YOLOX: CSPDarknet P5, YOLOXPAFPN, YOLOXHead; include/pcdm.h states the network) -----------------------------
// Everything that is not a dense convolution or the 5 x 5 maximum: image -> Focus tensor, nearest x 2 between channel slices, the per-prior decode
// and the greedy NMS; and pcdm_detect_forward, the whole schedule as one C call on one workspace.  The convolutions run on pcdm_conv2d_f32_act
// (eval_nets.hip), the SPP maxima on pcdm_maxpool5_f32 (pose_net.hip).  fp32 NHWC, channels in groups of four, no atomics, no allocation, no host
// synchronisation; every order is fixed, so reruns are bit-identical and an image's result does not depend on its place in the batch.
//
// The reference keeps score > 0.5 AFTER mmdet's NMS.  A greedy NMS in descending score order never lets a lower score suppress a higher one, so
// dropping the scores <= 0.5 BEFORE it leaves the same set above 0.5; the candidates here are filtered first.
namespace {
constexpr int kDetMaxCand = 1024;                 // candidates of one image that the NMS kernel holds in LDS
constexpr int kDetRegPitch = 8;                   // a head tensor's pixel: reg 0..3, obj 4, 5..7 zero, then the class logits

// out fp32 [N, S/2, S/2, 12] <- the Focus layout of the S x S canvas: the image resized to Wr x Hr (OpenCV's 8-bit INTER_LINEAR) top-left, 114
// elsewhere; channels (top-left, bottom-left, top-right, bottom-right) x (B, G, R).  One lane per Focus pixel.
__global__ __launch_bounds__(256) void detect_prep_kernel(const uint8_t* __restrict__ img, int H, int W, int Hr, int Wr, int S2, double scale_x,
                                                          double scale_y, int64_t total, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over (n, y / 2, x / 2)
    if (i >= total) return;
    const int x2 = (int)(i % S2), y2 = (int)((i / S2) % S2), n = (int)(i / ((int64_t)S2 * S2));
    float v[12];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int y = 2 * y2 + (p & 1), x = 2 * x2 + (p >> 1);
        if (x < Wr && y < Hr) {
            int xa, xb, a0, a1, ya, yb, b0, b1;
            cv_lin_coeff(x, scale_x, W, true, xa, xb, a0, a1);
            cv_lin_coeff(y, scale_y, H, false, ya, yb, b0, b1);
            const uint8_t* r0 = img + ((int64_t)n * H + ya) * W * 3;
            const uint8_t* r1 = img + ((int64_t)n * H + yb) * W * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int S0 = (int)r0[xa * 3 + c] * a0 + (int)r0[xb * 3 + c] * a1;
                const int S1 = (int)r1[xa * 3 + c] * a0 + (int)r1[xb * 3 + c] * a1;
                const int q = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
                v[p * 3 + 2 - c] = (float)imin(imax(q, 0), 255);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[p * 3 + c] = 114.0f;
        }
    }
    f32x4* o = (f32x4*)(out + i * 12);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = f32x4{v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
}

// nearest x 2: out[b, y, x, c] = x[b, y / 2, x / 2, c] between channel slices; one lane = one output pixel x four channels
__global__ __launch_bounds__(256) void upsample2_nearest_kernel(const float* __restrict__ x, int ldi, float* __restrict__ out, int ldo, int H, int W,
                                                                int C4, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over (b, y, x, c / 4) of the output
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    int64_t t = i / C4;
    const int64_t pix = t;
    const int px = (int)(t % (2 * W));
    t /= 2 * W;
    const int py = (int)(t % (2 * H)), b = (int)(t / (2 * H));
    *(f32x4*)(out + pix * ldo + 4 * c4) = *(const f32x4*)(x + (((int64_t)b * H + py / 2) * W + px / 2) * ldi + 4 * c4);
}

__device__ __forceinline__ float det_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

struct DetHeads { const float* p[3]; };

// YOLOXHead.predict_by_feat for prior i of image n (one lane each): head tensors fp32 [N, S/stride, S/stride, 8 + C4] = (reg 0..3, obj 4, classes from
// 8), priors in level order, row-major
__global__ __launch_bounds__(256) void detect_decode_kernel(DetHeads heads, int N, int S, int C, int ldh, int class_id, float score_thr, float sfx,
                                                            float sfy, int P, float* __restrict__ boxes, float* __restrict__ scores,
                                                            int32_t* __restrict__ labels, int32_t* __restrict__ cand) {
    const int i = blockIdx.x * 256 + threadIdx.x;                // over (n, prior)
    if (i >= N * P) return;
    const int n = i / P;
    int q = i % P, lvl = 0, hw = S / 8;
    while (q >= hw * hw) { q -= hw * hw; hw /= 2; ++lvl; }
    const float stride = (float)(8 << lvl), px = (float)(q % hw) * stride, py = (float)(q / hw) * stride;
    const float* h = heads.p[lvl] + ((int64_t)n * hw * hw + q) * ldh;
    const f32x4 reg = *(const f32x4*)h;
    const float cx = cv_mul(reg[0], stride) + px, cy = cv_mul(reg[1], stride) + py;
    const float hx = cv_mul(cv_mul(expf(reg[2]), stride), 0.5f), hy = cv_mul(cv_mul(expf(reg[3]), stride), 0.5f);
    float best = det_sigmoid(h[kDetRegPitch]);
    int lab = 0;
    for (int c = 1; c < C; ++c) {                                // torch.max: the first maximum; a NaN ranks highest
        const float v = det_sigmoid(h[kDetRegPitch + c]);
        if (best == best && (v > best || v != v)) { best = v; lab = c; }
    }
    const float sc = cv_mul(best, det_sigmoid(h[4]));
    *(f32x4*)(boxes + (int64_t)i * 4) = f32x4{(cx - hx) / sfx, (cy - hy) / sfy, (cx + hx) / sfx, (cy + hy) / sfy};
    scores[i] = sc;
    labels[i] = lab;
    cand[i] = lab == class_id && sc >= 0.01f && sc > score_thr ? 1 : 0;
}

struct DetBox { float x1, y1, x2, y2; };
__device__ __forceinline__ float det_area(const DetBox& a, float off) { return cv_mul(a.x2 - a.x1 + off, a.y2 - a.y1 + off); }
// mmcv's / mmpose's IoU: inter / (area a + area b - inter) with `off` on every width and height
__device__ __forceinline__ float det_iou(const DetBox& a, const DetBox& b, float off) {
    const float w = fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1) + off, h = fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1) + off;
    const float inter = cv_mul(w > 0.f ? w : 0.f, h > 0.f ? h : 0.f);
    return inter / (det_area(a, off) + det_area(b, off) - inter);
}

// One greedy pass over the flagged boxes of image n = blockIdx.x, in (score descending, index ascending) order.  The order is a rank by counting
// (no atomics): rank(i) = the flagged j with a higher score, or an equal one and j < i.  The best max_cand go to LDS; candidate r, if still
// kept, removes every later one whose IoU with it is > thr.  keep_out (or NULL): int32 [N, P] flags of the kept; out_* (or NULL): the first
// max_det kept in order, the rows behind them zero.
__global__ __launch_bounds__(256) void nms_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ flags,
                                                  int P, int max_cand, int max_det, float thr, float off, const int32_t* __restrict__ overflow_in,
                                                  int32_t* __restrict__ keep_out, float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                  int32_t* __restrict__ count, int32_t* __restrict__ overflow) {
    __shared__ DetBox sbox[kDetMaxCand];
    __shared__ float sscore[kDetMaxCand];
    __shared__ int sidx[kDetMaxCand], keep[kDetMaxCand], red[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* sc = scores + (int64_t)n * P;
    const int32_t* fl = flags + (int64_t)n * P;
    int mine = 0;
    for (int i = tid; i < P; i += 256) {
        const float si = sc[i];
        if (!fl[i] || si != si) continue;                         // (a NaN score is no candidate)
        int rank = 0;
        for (int j = 0; j < P; ++j) {
            const float sj = sc[j];
            rank += fl[j] && (sj > si || (sj == si && j < i)) ? 1 : 0;
        }
        ++mine;
        if (rank < max_cand) {
            const float* b = boxes + ((int64_t)n * P + i) * 4;
            sbox[rank] = DetBox{b[0], b[1], b[2], b[3]};
            sscore[rank] = si;
            sidx[rank] = i;
        }
    }
    red[tid] = mine;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (tid < m) red[tid] += red[tid + m];
        __syncthreads();
    }
    const int total = red[0], M = total < max_cand ? total : max_cand;
    for (int r = tid; r < M; r += 256) keep[r] = 1;
    __syncthreads();
    for (int r = 0; r + 1 < M; ++r) {
        if (keep[r]) {
            const DetBox a = sbox[r];
            for (int j = r + 1 + tid; j < M; j += 256)
                if (keep[j] && det_iou(a, sbox[j], off) > thr) keep[j] = 0;
        }
        __syncthreads();
    }
    if (tid == 0) {                                               // keep[r] <- 1 + the place of r among the kept
        int pos = 0;
        for (int r = 0; r < M; ++r) keep[r] = keep[r] ? ++pos : 0;
        red[0] = pos;
    }
    if (keep_out)
        for (int i = tid; i < P; i += 256) keep_out[(int64_t)n * P + i] = 0;
    __syncthreads();
    const int kept = red[0], nout = kept < max_det ? kept : max_det;
    for (int r = tid; r < M; r += 256) {
        const int pos = keep[r] - 1;
        if (pos < 0 || pos >= max_det) continue;
        if (keep_out) keep_out[(int64_t)n * P + sidx[r]] = 1;
        if (out_boxes) {
            *(f32x4*)(out_boxes + ((int64_t)n * max_det + pos) * 4) = f32x4{sbox[r].x1, sbox[r].y1, sbox[r].x2, sbox[r].y2};
            out_scores[(int64_t)n * max_det + pos] = sscore[r];
        }
    }
    if (out_boxes)
        for (int d = nout + tid; d < max_det; d += 256) {
            *(f32x4*)(out_boxes + ((int64_t)n * max_det + d) * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
            out_scores[(int64_t)n * max_det + d] = 0.f;
        }
    if (tid == 0) {
        if (count) count[n] = nout;
        if (overflow) overflow[n] = (total > max_cand || kept > max_det || (overflow_in && overflow_in[n])) ? 1 : 0;
    }
}

inline bool det_slice_ok(int C, int ld, int off) { return C > 0 && C % 4 == 0 && ld % 4 == 0 && off >= 0 && off % 4 == 0 && ld >= C && off <= ld - C; }
inline int det_priors(int S) { return 21 * (S / 32) * (S / 32); }
inline bool det_size_ok(int S) { return S >= 32 && S <= 4096 && S % 32 == 0; }
}  // namespace

extern "C" int pcdm_detect_resized(int H, int W, int S, int* Hr, int* Wr) {
    if (H <= 0 || W <= 0 || H > 32768 || W > 32768 || !det_size_ok(S)) return -1;
    const double f = (double)S / (double)(H > W ? H : W);
    const int wr = (int)((double)W * f + 0.5), hr = (int)((double)H * f + 0.5);
    if (wr < 1 || hr < 1 || wr > S || hr > S) return -1;         // (a side thinner than 1 / (2 f) pixels would vanish)
    if (Hr) *Hr = hr;
    if (Wr) *Wr = wr;
    return 0;
}

extern "C" int pcdm_detect_prep(const void* images, int N, int H, int W, int S, float* out, pcdm_stream_t s) {
    int Hr, Wr;
    if (!images || !out || ((uintptr_t)out & 15) || N <= 0 || pcdm_detect_resized(H, W, S, &Hr, &Wr)) return -1;
    const int64_t total = (int64_t)N * (S / 2) * (S / 2);
    if ((int64_t)N * H * W * 3 >= (int64_t)1 << 31 || total * 12 >= (int64_t)1 << 31) return -1;
    const double scale_x = 1.0 / ((double)Wr / (double)W), scale_y = 1.0 / ((double)Hr / (double)H);
    PCDM_LAUNCH(detect_prep_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, (const uint8_t*)images, H, W, Hr, Wr, S / 2, scale_x, scale_y, total,
                out);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_upsample2_nearest_f32(const float* x, int B, int H, int W, int C, int in_pitch, int in_offset, float* out, int out_pitch,
                                          int out_offset, pcdm_stream_t s) {
    if (!x || !out || B <= 0 || H <= 0 || W <= 0 || !det_slice_ok(C, in_pitch, in_offset) || !det_slice_ok(C, out_pitch, out_offset)) return -1;
    if (((uintptr_t)x | (uintptr_t)out) & 15) return -1;
    if (x == out && in_pitch == out_pitch && in_offset < out_offset + C && out_offset < in_offset + C) return -1;   // overlapping slices of one tensor
    if ((int64_t)B * H * W * in_pitch >= (int64_t)1 << 31 || (int64_t)B * H * W * 4 * out_pitch >= (int64_t)1 << 31) return -1;
    const int64_t total = (int64_t)B * H * W * 4 * (C / 4);
    PCDM_LAUNCH(upsample2_nearest_kernel, grid1d(total, 256), dim3(256), 0, (hipStream_t)s, x + in_offset, in_pitch, out + out_offset, out_pitch, H, W,
                C / 4, total);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_detect_decode(const float* head8, const float* head16, const float* head32, int N, int S, int num_classes, int class_id,
                                  float score_thr, int H, int W, float* boxes, float* scores, int32_t* labels, int32_t* candidates, pcdm_stream_t s) {
    int Hr, Wr;
    if (!head8 || !head16 || !head32 || !boxes || !scores || !labels || !candidates || N <= 0 || num_classes <= 0 || num_classes > 1024 ||
        class_id < 0 || class_id >= num_classes || !(score_thr == score_thr) || pcdm_detect_resized(H, W, S, &Hr, &Wr))
        return -1;
    if (((uintptr_t)head8 | (uintptr_t)head16 | (uintptr_t)head32 | (uintptr_t)boxes) & 15) return -1;
    const int P = det_priors(S), ldh = kDetRegPitch + (num_classes + 3) / 4 * 4;
    if ((int64_t)N * P >= (int64_t)1 << 24 || (int64_t)N * (S / 8) * (S / 8) * ldh >= (int64_t)1 << 31) return -1;
    const float sfx = (float)((double)Wr / (double)W), sfy = (float)((double)Hr / (double)H);
    PCDM_LAUNCH(detect_decode_kernel, grid1d((int64_t)N * P, 256), dim3(256), 0, (hipStream_t)s, DetHeads{{head8, head16, head32}}, N, S, num_classes, ldh,
                class_id, score_thr, sfx, sfy, P, boxes, scores, labels, candidates);
    PCDM_CHECK_LAUNCH();
    return 0;
}

extern "C" int pcdm_nms_f32(const float* boxes, const float* scores, const int32_t* flags, int N, int P, int max_candidates, int max_det, float thr,
                            float offset, const int32_t* overflow_in, int32_t* keep, float* out_boxes, float* out_scores, int32_t* count,
                            int32_t* overflow, pcdm_stream_t s) {
    if (!boxes || !scores || !flags || N <= 0 || N > 65535 || P <= 0 || (int64_t)N * P >= (int64_t)1 << 24 || max_candidates <= 0 ||
        max_candidates > kDetMaxCand || max_det <= 0 || max_det > max_candidates || !(thr == thr) || !(offset == offset))
        return -1;
    if ((out_boxes != nullptr) != (out_scores != nullptr) || (!keep && !out_boxes) || keep == flags || ((uintptr_t)out_boxes & 15)) return -1;
    PCDM_LAUNCH(nms_kernel, dim3(N), dim3(256), 0, (hipStream_t)s, boxes, scores, flags, P, max_candidates, max_det, thr, offset, overflow_in, keep,
                out_boxes, out_scores, count, overflow);
    PCDM_CHECK_LAUNCH();
    return 0;
}

// ---- the whole schedule as one C call (as pcdm_dwpose_forward): prep -> backbone -> neck -> head -> decode -> two NMS passes ----------------------
namespace {
struct DetLayout {
    // byte offsets: the Focus tensor | x0, x1 (the backbone's running tensor) | cat, t (a CSP layer's concatenation and block intermediate) | spp |
    // the neck's four concatenations | c5, t4, p3, p4, p5 | the out_convs' maps | a head branch's two intermediates | the head tensors | decode, NMS
    int64_t focus, x[2], cat, t, spp, td0, td1, bu0, bu1, c5, t4, p3, p4, p5, f[3], hb[2], head[3], box, score, label, cand, keep, ovf, total;
    struct { const char* name; int64_t off, bytes; } ent[29];   // every buffer in offset order (pcdm_detect_ws_layout)
    int n_ent;
};
inline int64_t det_align(int64_t elems) { return (elems * (int64_t)sizeof(float) + 255) / 256 * 256; }
inline bool detect_cfg_ok(const pcdm_detect_config* c) {
    if (!c || !det_size_ok(c->S) || c->num_classes <= 0 || c->num_classes > 1024 || c->class_id < 0 || c->class_id >= c->num_classes) return false;
    if (c->stem <= 0 || c->stem % 8 || c->head <= 0 || c->head % 8 || c->neck_blocks <= 0 || c->neck_blocks > 64) return false;
    for (int s = 0; s < 4; ++s)
        if (c->out[s] <= 0 || c->out[s] % 8 || c->out[s] > 1 << 16 || c->blocks[s] <= 0 || c->blocks[s] > 64) return false;
    if (c->max_candidates <= 0 || c->max_candidates > kDetMaxCand || c->max_det <= 0 || c->max_det > c->max_candidates) return false;
    return c->score_thr == c->score_thr && c->nms_thr == c->nms_thr && c->pose_nms_thr == c->pose_nms_thr;
}
inline int detect_n_conv(const pcdm_detect_config* c) {
    int n = 1 + 2 + 2 + 2 + 3 + 18 + 4 * (2 + 2 * c->neck_blocks);   // stem; SPP; reduce, downsamples, out_convs; the head; the neck's CSP layers
    for (int s = 0; s < 4; ++s) n += 3 + 2 * c->blocks[s];
    return n;
}
inline bool detect_layout(const pcdm_detect_config* c, int N, DetLayout* o) {
    if (!detect_cfg_ok(c) || N <= 0 || N > 4096) return false;
    const int64_t S = c->S, B = N, p2 = B * (S / 2) * (S / 2), p4 = p2 / 4, p8 = p4 / 4, p16 = p8 / 4, p32 = p16 / 4;
    const int64_t o0 = c->out[0], o1 = c->out[1], o2 = c->out[2], o3 = c->out[3];
    const int64_t ldh = kDetRegPitch + (c->num_classes + 3) / 4 * 4, P = det_priors(c->S);
    int64_t x = p2 * c->stem, cat = 0;
    const int64_t xs[] = {p4 * o0, p8 * o1, p16 * o2, p32 * o3}, cats[] = {p4 * o0, p8 * o1, p16 * o2, p32 * o3, p16 * o2, p8 * o1, p16 * o2, p32 * o3};
    for (int64_t v : xs) x = v > x ? v : x;
    for (int64_t v : cats) cat = v > cat ? v : cat;
    if (x >= (int64_t)1 << 31 || cat >= (int64_t)1 << 31 || p8 * 2 * o1 >= (int64_t)1 << 31 || p16 * 2 * o2 >= (int64_t)1 << 31 || p2 * 12 >= (int64_t)1 << 31 ||
        p8 * ldh >= (int64_t)1 << 31 || p8 * c->head >= (int64_t)1 << 31 || B * P >= (int64_t)1 << 24)
        return false;
    int64_t at = 0;
    const int64_t redzone = pcdm_get_workspace_redzone();   // (test hook: bytes left unused behind every buffer; 0 in product use)
    o->n_ent = 0;
    auto take = [&](const char* name, int64_t elems) {
        const int64_t here = at;
        o->ent[o->n_ent++] = {name, here, det_align(elems)};
        at += det_align(elems) + redzone;
        return here;
    };
    o->focus = take("focus", p2 * 12);
    o->x[0] = take("x0", x); o->x[1] = take("x1", x);
    o->cat = take("cat", cat); o->t = take("t", (cat + 1) / 2);
    o->spp = take("spp", p32 * 2 * o3);
    o->td0 = take("td0", p16 * 2 * o2); o->td1 = take("td1", p8 * 2 * o1); o->bu0 = take("bu0", p16 * 2 * o1); o->bu1 = take("bu1", p32 * 2 * o2);
    o->c5 = take("c5", p32 * o3); o->t4 = take("t4", p16 * o2); o->p3 = take("p3", p8 * o1); o->p4 = take("p4", p16 * o2); o->p5 = take("p5", p32 * o3);
    o->f[0] = take("f0", p8 * c->head); o->f[1] = take("f1", p16 * c->head); o->f[2] = take("f2", p32 * c->head);
    o->hb[0] = take("hb0", p8 * c->head); o->hb[1] = take("hb1", p8 * c->head);
    o->head[0] = take("head0", p8 * ldh); o->head[1] = take("head1", p16 * ldh); o->head[2] = take("head2", p32 * ldh);
    o->box = take("box", B * P * 4); o->score = take("score", B * P); o->label = take("label", B * P); o->cand = take("cand", B * P);
    o->keep = take("keep", B * P); o->ovf = take("ovf", B);
    o->total = at;
    return true;
}
}  // namespace

extern "C" int64_t pcdm_detect_ws_bytes(const pcdm_detect_config* cfg, int N) {
    DetLayout lay;
    return detect_layout(cfg, N, &lay) ? lay.total : -1;
}

extern "C" int pcdm_detect_ws_layout(const pcdm_detect_config* cfg, int N, int index, const char** name, int64_t* offset, int64_t* bytes) {
    DetLayout lay;
    if (!detect_layout(cfg, N, &lay)) return -1;
    if (index == -1) return lay.n_ent;
    if (index < 0 || index >= lay.n_ent) return -1;
    if (name) *name = lay.ent[index].name;
    if (offset) *offset = lay.ent[index].off;
    if (bytes) *bytes = lay.ent[index].bytes;
    return lay.n_ent;
}

extern "C" int pcdm_detect_forward(const void* images, int N, int H, int W, const pcdm_detect_config* cfg, const pcdm_detect_weights* wts, float* boxes,
                                   float* scores, int32_t* count, int32_t* overflow, void* ws, int64_t ws_bytes, pcdm_stream_t s) {
    DetLayout lay;
    if (!images || !wts || !boxes || !scores || !count || !overflow || !ws || ((uintptr_t)ws & 15) || ((uintptr_t)boxes & 15) ||
        !detect_layout(cfg, N, &lay) || ws_bytes < lay.total || pcdm_detect_resized(H, W, cfg->S, nullptr, nullptr) ||
        (int64_t)N * H * W * 3 >= (int64_t)1 << 31)
        return -1;
    const int n_conv = detect_n_conv(cfg);
    if (!wts->conv_w || !wts->conv_b || wts->n_conv != n_conv) return -1;
    for (int i = 0; i < n_conv; ++i)
        if (!wts->conv_w[i] || !wts->conv_b[i]) return -1;
    char* base = (char*)ws;
    auto buf = [&](int64_t off) { return (float*)(base + off); };
    const int silu = 2, S = cfg->S, hc = cfg->head, C4 = (cfg->num_classes + 3) / 4 * 4, ldh = kDetRegPitch + C4;
    const int o0 = cfg->out[0], o1 = cfg->out[1], o2 = cfg->out[2], o3 = cfg->out[3];
    int ci = 0, rc;
    // conv: the next packed convolution of the schedule, channels [ioff, ioff + cin) of x [N, h, w, ldi] -> channels [off, off + cout) of out [N, ho, wo, ldo]
    auto conv = [&](const float* x, int h, int w, int cin, int ldi, int ioff, int cout, int k, int stride, int act, const float* res, int ldr, float* out,
                    int ldo, int off) {
        const int i = ci++;
        return pcdm_conv2d_f32_act(x, N, h, w, cin, ldi, ioff, wts->conv_w[i], wts->conv_b[i], cout, k, k, stride, k / 2, k / 2, act, res, ldr, 0, nullptr,
                                   out, ldo, off, s);
    };
    // csp: a CSP layer on channels [ioff, ioff + cin) of x: (main | short) as one convolution into `cat`, the blocks on the main half in place, final_conv
    auto csp = [&](const float* x, int h, int w, int cin, int ldi, int ioff, int cout, int blocks, bool ident, float* out, int ldo, int off) {
        const int mid = cout / 2;
        float* cat = buf(lay.cat);
        int r;
        if ((r = conv(x, h, w, cin, ldi, ioff, 2 * mid, 1, 1, silu, nullptr, 0, cat, 2 * mid, 0))) return r;
        for (int b = 0; b < blocks; ++b) {
            if ((r = conv(cat, h, w, mid, 2 * mid, 0, mid, 1, 1, silu, nullptr, 0, buf(lay.t), mid, 0))) return r;
            if ((r = conv(buf(lay.t), h, w, mid, mid, 0, mid, 3, 1, silu, ident ? cat : nullptr, 2 * mid, cat, 2 * mid, 0))) return r;
        }
        return conv(cat, h, w, 2 * mid, 2 * mid, 0, cout, 1, 1, silu, nullptr, 0, out, ldo, off);
    };
    if ((rc = pcdm_detect_prep(images, N, H, W, S, buf(lay.focus), s))) return rc;
    const int s2 = S / 2, s4 = S / 4, s8 = S / 8, s16 = S / 16, s32 = S / 32;
    float *x0 = buf(lay.x[0]), *x1 = buf(lay.x[1]), *td0 = buf(lay.td0), *td1 = buf(lay.td1), *bu0 = buf(lay.bu0), *bu1 = buf(lay.bu1);
    float *spp = buf(lay.spp), *c5 = buf(lay.c5), *t4 = buf(lay.t4), *p3 = buf(lay.p3), *p4 = buf(lay.p4), *p5 = buf(lay.p5);
    if ((rc = conv(buf(lay.focus), s2, s2, 12, 12, 0, cfg->stem, 3, 1, silu, nullptr, 0, x0, cfg->stem, 0))) return rc;
    if ((rc = conv(x0, s2, s2, cfg->stem, cfg->stem, 0, o0, 3, 2, silu, nullptr, 0, x1, o0, 0))) return rc;
    if ((rc = csp(x1, s4, s4, o0, o0, 0, o0, cfg->blocks[0], true, x0, o0, 0))) return rc;
    if ((rc = conv(x0, s4, s4, o0, o0, 0, o1, 3, 2, silu, nullptr, 0, x1, o1, 0))) return rc;
    if ((rc = csp(x1, s8, s8, o1, o1, 0, o1, cfg->blocks[1], true, td1, 2 * o1, o1))) return rc;              // c3: the second half of td1's concatenation
    if ((rc = conv(td1, s8, s8, o1, 2 * o1, o1, o2, 3, 2, silu, nullptr, 0, x1, o2, 0))) return rc;
    if ((rc = csp(x1, s16, s16, o2, o2, 0, o2, cfg->blocks[2], true, td0, 2 * o2, o2))) return rc;            // c4: the second half of td0's
    if ((rc = conv(td0, s16, s16, o2, 2 * o2, o2, o3, 3, 2, silu, nullptr, 0, x1, o3, 0))) return rc;
    if ((rc = conv(x1, s32, s32, o3, o3, 0, o3 / 2, 1, 1, silu, nullptr, 0, spp, 2 * o3, 0))) return rc;
    for (int j = 0; j < 3; ++j)
        if ((rc = pcdm_maxpool5_f32(spp, N, s32, s32, o3 / 2, 2 * o3, j * (o3 / 2), spp, 2 * o3, (j + 1) * (o3 / 2), s))) return rc;
    if ((rc = conv(spp, s32, s32, 2 * o3, 2 * o3, 0, o3, 1, 1, silu, nullptr, 0, x0, o3, 0))) return rc;
    if ((rc = csp(x0, s32, s32, o3, o3, 0, o3, cfg->blocks[3], false, c5, o3, 0))) return rc;
    // the neck: every tensor that feeds a concatenation is written into its slice
    if ((rc = conv(c5, s32, s32, o3, o3, 0, o2, 1, 1, silu, nullptr, 0, bu1, 2 * o2, o2))) return rc;          // r5
    if ((rc = pcdm_upsample2_nearest_f32(bu1, N, s32, s32, o2, 2 * o2, o2, td0, 2 * o2, 0, s))) return rc;
    if ((rc = csp(td0, s16, s16, 2 * o2, 2 * o2, 0, o2, cfg->neck_blocks, false, t4, o2, 0))) return rc;
    if ((rc = conv(t4, s16, s16, o2, o2, 0, o1, 1, 1, silu, nullptr, 0, bu0, 2 * o1, o1))) return rc;          // r4
    if ((rc = pcdm_upsample2_nearest_f32(bu0, N, s16, s16, o1, 2 * o1, o1, td1, 2 * o1, 0, s))) return rc;
    if ((rc = csp(td1, s8, s8, 2 * o1, 2 * o1, 0, o1, cfg->neck_blocks, false, p3, o1, 0))) return rc;
    if ((rc = conv(p3, s8, s8, o1, o1, 0, o1, 3, 2, silu, nullptr, 0, bu0, 2 * o1, 0))) return rc;
    if ((rc = csp(bu0, s16, s16, 2 * o1, 2 * o1, 0, o2, cfg->neck_blocks, false, p4, o2, 0))) return rc;
    if ((rc = conv(p4, s16, s16, o2, o2, 0, o2, 3, 2, silu, nullptr, 0, bu1, 2 * o2, 0))) return rc;
    if ((rc = csp(bu1, s32, s32, 2 * o2, 2 * o2, 0, o3, cfg->neck_blocks, false, p5, o3, 0))) return rc;
    const float* pl[3] = {p3, p4, p5};
    const int pc[3] = {o1, o2, o3}, ps[3] = {s8, s16, s32};
    for (int l = 0; l < 3; ++l)
        if ((rc = conv(pl[l], ps[l], ps[l], pc[l], pc[l], 0, hc, 1, 1, silu, nullptr, 0, buf(lay.f[l]), hc, 0))) return rc;
    for (int l = 0; l < 3; ++l) {
        float *f = buf(lay.f[l]), *a = buf(lay.hb[0]), *b = buf(lay.hb[1]), *head = buf(lay.head[l]);
        if ((rc = conv(f, ps[l], ps[l], hc, hc, 0, hc, 3, 1, silu, nullptr, 0, a, hc, 0))) return rc;
        if ((rc = conv(a, ps[l], ps[l], hc, hc, 0, hc, 3, 1, silu, nullptr, 0, b, hc, 0))) return rc;
        if ((rc = conv(b, ps[l], ps[l], hc, hc, 0, C4, 1, 1, 0, nullptr, 0, head, ldh, kDetRegPitch))) return rc;       // the class logits
        if ((rc = conv(f, ps[l], ps[l], hc, hc, 0, hc, 3, 1, silu, nullptr, 0, a, hc, 0))) return rc;
        if ((rc = conv(a, ps[l], ps[l], hc, hc, 0, hc, 3, 1, silu, nullptr, 0, b, hc, 0))) return rc;
        if ((rc = conv(b, ps[l], ps[l], hc, hc, 0, kDetRegPitch, 1, 1, 0, nullptr, 0, head, ldh, 0))) return rc;        // reg and obj as one
    }
    const int P = det_priors(S);
    int32_t *label = (int32_t*)buf(lay.label), *cand = (int32_t*)buf(lay.cand), *keep = (int32_t*)buf(lay.keep), *ovf = (int32_t*)buf(lay.ovf);
    if ((rc = pcdm_detect_decode(buf(lay.head[0]), buf(lay.head[1]), buf(lay.head[2]), N, S, cfg->num_classes, cfg->class_id, cfg->score_thr, H, W,
                                 buf(lay.box), buf(lay.score), label, cand, s)))
        return rc;
    if ((rc = pcdm_nms_f32(buf(lay.box), buf(lay.score), cand, N, P, cfg->max_candidates, cfg->max_candidates, cfg->nms_thr, 0.0f, nullptr, keep, nullptr,
                           nullptr, nullptr, ovf, s)))
        return rc;
    return pcdm_nms_f32(buf(lay.box), buf(lay.score), keep, N, P, cfg->max_candidates, cfg->max_det, cfg->pose_nms_thr, 1.0f, ovf, nullptr, boxes, scores,
                        count, overflow, s);
}
