// The UNet forward as ONE C entry: pcdm_unet_forward(ctx, ...) (SURVEY.md §8b "fused unet_forward(ctx, ...)" + opaque ctx).
//
// Host code only -- a schedule of calls into the kernels of this library, the C++ twin of pcdms_amd/unet.py::_forward_nhwc /
// prepare_conditioning (which follow /root/reference/src/models/stage2_inpaint_unet_2d_condition.py:579-825 and the diffusers 0.24.0
// blocks of SURVEY.md Appendix A).  A host without Python builds a pcdm_unet from a topology description, registers the packed
// weights by their diffusers module paths (pcdm_pack_* produce the layouts from fp32 host tensors), hands over ONE workspace, and runs
// prepare_conditioning once per sampling call and forward once per denoise step; nothing is allocated inside, every launch goes to the
// caller's stream, all scratch addresses are fixed by the plan (the whole step is capturable in a hipGraph).
// The Python package keeps its own schedule (autotuning, fp8 attention, emulator tests); tests/test_unet_ctx.py holds the two to
// bit-identical outputs.
#include "pcdm_device.h"
#include "../../include/pcdm.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

namespace {
struct PW {   // a packed weight as pcdm_gemm wants it
    const void* w = nullptr;
    const float* bias = nullptr;
    const float* wsum = nullptr;   // row sums of LayerNorm-folded weights (pcdm_gemm_params.ln_wsum)
    int N = 0, K = 0, Npad = 0, cin = 0;
};
struct Vec {
    const float* v = nullptr;
    int n = 0;
};
typedef std::tuple<int, int, int, int, int, int, int, int, int, int, int> TileKey;   // ln, M, Npad, K, conv, stride, upsample, epilogue, two-source, residual, zero_rows

struct Buf {
    int64_t off = 0, bytes = 0;
};
}  // namespace

struct pcdm_unet {
    pcdm_unet_config cfg;
    std::map<std::string, PW> w;
    std::map<std::string, Vec> v;
    std::map<TileKey, std::pair<int, int>> tiles;
    // plan (valid for plan_key)
    std::tuple<int, int, int, int, int64_t, int> plan_key{0, 0, 0, 0, 0, 0};   // B, h, w, L, the red-zone size it was laid out with, FreeU on
    std::map<std::string, Buf> bufs;
    std::vector<std::string> order;   // the names of bufs in offset order (pcdm_unet_workspace_layout)
    int64_t ws_bytes = 0;
    // per WORKSPACE: what the last prepare_conditioning on it was given -- the shape, n0 = leading batch entries with an all-zero context, pose_b.
    // forward() takes n0 from the workspace it runs on (a host may alternate workspaces / batch shapes on one context) and refuses a
    // workspace whose conditioning was never prepared or was prepared for another batch / pose layout
    struct WsCond {
        int B = 0, h = 0, w = 0, L = 0, n0 = 0, pose_b = 0, shared = 0;
        const float* time_table = nullptr;   // [steps][B][sum Cout] fp32 (pcdm_unet_prepare_timesteps), caller-owned
        int time_steps = 0;
        const void* time_t_dev = nullptr;    // the int64 or float timestep table the time table was computed for
    };
    std::map<const void*, WsCond> cond_of_ws;
    bool attn_fp8 = false;   // every attention with e4m3 K / V^T / Q / P operands (pcdm_unet_set_attention_fp8; BASELINE.json configs[4])
    bool freeu = false;      // pcdm_freeu in front of every resnet of up blocks 0 and 1 (pcdm_unet_set_freeu): {s1, s2}, {b1, b2}
    float fu_s[2] = {1.f, 1.f}, fu_b[2] = {1.f, 1.f};
    std::string err;
};

namespace {
constexpr int64_t kAlign = 256;
constexpr int64_t kSplitKFloats = 1 << 24;   // split-K workspace (fp32), as pcdms_amd.ops._splitk_ws

int64_t g_redzone = 0;   // pcdm_set_workspace_redzone: bytes left unused behind every buffer a layout carves (test hook, include/pcdm.h)

int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
bool getenv_off(const char* name) {   // A/B switches shared with pcdms_amd.ops ("0" = off)
    const char* e = getenv(name);
    return e && e[0] == '0';
}

struct Planner {
    pcdm_unet* u;
    int64_t off = 0;
    void add(const std::string& name, int64_t bytes) {
        auto it = u->bufs.find(name);
        if (it != u->bufs.end()) {   // same name, larger use: grow in place only while it is the last buffer; otherwise keep the max up front
            if (it->second.bytes >= bytes) return;
        }
        Buf b;
        b.off = off;
        b.bytes = round_up(bytes, kAlign);
        off += b.bytes + g_redzone;
        u->bufs[name] = b;
        u->order.push_back(name);
    }
};

std::vector<std::tuple<std::string, int, int, int>> resnets(const pcdm_unet_config& c) {   // (prefix, cin, cout, level)
    std::vector<std::tuple<std::string, int, int, int>> r;
    const int n = c.n_levels, L = c.layers_per_block;
    int out = c.block_out_channels[0];
    for (int i = 0; i < n; ++i) {
        const int cin = out;
        out = c.block_out_channels[i];
        for (int j = 0; j < L; ++j) r.emplace_back("down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j) + ".", j == 0 ? cin : out, out, i);
    }
    r.emplace_back("mid_block.resnets.0.", c.block_out_channels[n - 1], c.block_out_channels[n - 1], n - 1);
    r.emplace_back("mid_block.resnets.1.", c.block_out_channels[n - 1], c.block_out_channels[n - 1], n - 1);
    out = c.block_out_channels[n - 1];
    for (int i = 0; i < n; ++i) {
        const int prev = out;
        out = c.block_out_channels[n - 1 - i];
        const int inc = c.block_out_channels[n - 1 - (i + 1 < n ? i + 1 : n - 1)];
        for (int j = 0; j < L + 1; ++j) {
            const int skip = j == L ? inc : out, rin = j == 0 ? prev : out;
            r.emplace_back("up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j) + ".", rin + skip, out, n - 1 - i);
        }
    }
    return r;
}

// time-embedding column offset of every resnet inside the concatenated time_emb_proj (registration order == resnets())
std::map<std::string, int> temb_offsets(const pcdm_unet_config& c, int* total) {
    std::map<std::string, int> m;
    int off = 0;
    for (auto& r : resnets(c)) {
        m[std::get<0>(r)] = off;
        off += std::get<2>(r);
    }
    *total = off;
    return m;
}

struct Run {   // one forward / conditioning pass: helpers around the C-ABI calls
    pcdm_unet* u;
    char* ws;
    pcdm_stream_t st;
    int rc = 0;

    template <typename T = void>
    T* buf(const std::string& name) {
        auto it = u->bufs.find(name);
        if (it == u->bufs.end()) {
            u->err = "no buffer " + name;
            rc = -1;
            return nullptr;
        }
        return (T*)(ws + it->second.off);
    }
    const PW* pw(const std::string& name) {
        auto it = u->w.find(name);
        if (it == u->w.end()) {
            u->err = "weight not registered: " + name;
            rc = -1;
            return nullptr;
        }
        return &it->second;
    }
    const float* vec(const std::string& name) {
        auto it = u->v.find(name);
        if (it == u->v.end()) {
            u->err = "vector not registered: " + name;
            rc = -1;
            return nullptr;
        }
        return it->second.v;
    }
    void chk(int r, const char* what) {
        if (r != 0 && rc == 0) {
            rc = r;
            u->err = std::string(what) + " failed";
        }
    }

    struct G {   // optional arguments of gemm()
        const void* a2 = nullptr;
        int64_t lda2 = 0;
        const void* a3 = nullptr;   // conv with extra K (pcdm_gemm_params.a3): a2 [M, c1] and a3 [M, cx - c1] are the 1x1 sources behind the taps
        int64_t lda3 = 0;
        int c1 = 0;                 // ... and c1 the channels a2 supplies (0: linear two-source, c1 = lda)
        const float* rowvec = nullptr;
        int64_t ldrv = 0;
        int rows_per_batch = 0;
        const void* residual = nullptr;
        int64_t ldr = 0;
        int res_mod = 0;
        int epilogue = PCDM_EPI_STORE;
        void* out2 = nullptr;
        int64_t ldo2 = 0;
        int vt_col0 = 0;
        int conv = 0, B = 0, Hi = 0, Wi = 0, Ho = 0, Wo = 0, stride = 1, upsample = 0;
        uint64_t tap_lut = 0;      // conv over a subset of the nine taps per output-channel group (pcdm_gemm_params.tap_lut / tap_group_n)
        int tap_group_n = 0;
        int zero_rows = 0;
        int64_t ldo = 0;   // 0: N (GEGLU / NCHW: N)
        const PW* ln = nullptr;   // LayerNorm-folded twin of the weight (rowgemm tiles, or the tiled kernel with in-kernel statistics / producer partials)
        float ln_eps = 0.f;
        int dup_rows = 0;   // pcdm_gemm_params.dup_rows
        const int32_t* rowvec_step = nullptr;   // pcdm_gemm_params.rowvec_step / rowvec_step_stride / rowvec_step_count / step_error
        int64_t rowvec_step_stride = 0;
        int rowvec_step_count = 0;
        int32_t* step_error = nullptr;
        int defer = 0;   // split-K only: 1 = leave the reduce to the GroupNorm that reads `out` next (and let it write `out`), 2 = ... not write it
        float* row_stats = nullptr;   // producer: write the LayerNorm partials of the stored rows here when the tile in use can (pcdm_gemm_params.row_stats_out);
                                      // consumer (gemm_ln): the partials of the A rows (used when stats_valid and the table asks for mode 2)
    };
    bool stats_valid = false;   // did the last gemm() that was handed G::row_stats write them?
    // the split-K GEMM whose reduce is still pending (pcdm_gemm_params.defer_reduce): consumed by the next groupnorm() on its `out`
    pcdm_gn_splitk_src pend;
    const void* pend_out = nullptr;
    // out = epilogue(A W^T): the parameter block pcdms_amd.ops.gemm builds, the tile from the registered table (0 = library heuristic)
    void gemm(const void* a, int64_t lda, int M, const PW* w, void* out, const G& g) {
        if (rc || !w) return;
        pcdm_gemm_params p;
        memset(&p, 0, sizeof(p));
        p.struct_size = (uint32_t)sizeof(p);
        p.a = a;
        p.lda = lda;
        p.c1 = g.c1 ? g.c1 : (g.a2 ? (int)lda : w->K);
        p.a2 = g.a2;
        p.lda2 = g.lda2;
        p.a3 = g.a3;
        p.lda3 = g.lda3;
        p.tap_lut = g.tap_lut;
        p.tap_group_n = g.tap_group_n;
        p.conv = g.conv;
        if (g.conv) {
            p.B = g.B; p.Hi = g.Hi; p.Wi = g.Wi; p.Ho = g.Ho; p.Wo = g.Wo;
            p.stride = g.stride; p.upsample = g.upsample; p.cin = w->cin;
        }
        p.w = w->w;
        p.M = M; p.N = w->N; p.K = w->K; p.Npad = w->Npad;
        p.bias = w->bias;
        p.rowvec = g.rowvec;
        p.ldrv = g.ldrv;
        p.rows_per_batch = g.rows_per_batch ? g.rows_per_batch : M;
        p.residual = g.residual;
        p.ldr = g.residual ? (g.ldr ? g.ldr : w->N) : 0;
        p.res_mod = g.res_mod;
        p.epilogue = g.epilogue;
        p.vt_col0 = g.vt_col0;
        p.out = out;
        p.ldo = g.ldo ? g.ldo : w->N;
        p.out2 = g.out2;
        p.ldo2 = g.ldo2;
        p.zero_rows = g.zero_rows;
        p.dup_rows = g.dup_rows;
        p.rowvec_step = g.rowvec ? g.rowvec_step : nullptr;
        p.rowvec_step_stride = g.rowvec_step_stride;
        p.rowvec_step_count = g.rowvec_step_count;
        p.step_error = g.step_error;
        const TileKey key{0, M, w->Npad, w->K, g.conv, g.conv ? g.stride + (g.tap_group_n ? 20 : 0) : 0, g.upsample, g.epilogue, g.a2 ? 1 : 0, g.residual ? 1 : 0, g.zero_rows ? 1 : (g.dup_rows ? 2 : 0)};
        auto it = u->tiles.find(key);
        // (a table entry that names the A-in-registers kernel for a call it cannot serve -- row vector, fewer residual rows than M -- is skipped:
        //  the key does not carry those; pcdms_amd.ops.gemm does the same)
        if (it != u->tiles.end() && !(it->second.first >= 31 /* the A-in-registers tiles: pcdm.h */ && (g.rowvec || (g.residual && g.res_mod < M)))) {
            p.tile = it->second.first;
            if (it->second.second > 1) {
                p.split_k = it->second.second;
                p.ws = buf<float>("splitk");
                p.ws_floats = kSplitKFloats;
                if ((int64_t)p.split_k * M * w->Npad > kSplitKFloats) { p.split_k = 0; p.tile = 0; p.ws = nullptr; p.ws_floats = 0; }
            }
        }
        if (g.row_stats) {   // (pcdms_amd.ops.gemm(row_stats=): the same condition, so that both schedules launch the same instances)
            const int tl = p.tile;
            stats_valid = (tl == 2 || tl == 4 || tl == 5 || tl == 6 || tl == 7 || tl == 8 || tl == 10 || tl == 18) && p.split_k <= 1 && !g.conv &&
                          g.epilogue == PCDM_EPI_STORE && w->N % 32 == 0;
            if (stats_valid) p.row_stats_out = g.row_stats;
        } else {
            stats_valid = false;   // (a launch that was not asked for partials invalidates the ones an earlier launch left: ADVICE r5)
        }
        if (pend_out) { rc = -1; u->err = "a deferred split-K reduce was never consumed"; return; }
        if (g.defer && p.split_k > 1 && g.epilogue == PCDM_EPI_STORE && p.ldo == w->N && (!g.residual || g.res_mod == M || g.res_mod == 0) &&
            !getenv_off("PCDM_DEFER_SPLITK")) {
            p.defer_reduce = 1;
            memset(&pend, 0, sizeof(pend));
            pend.struct_size = (uint32_t)sizeof(pend);
            pend.part = p.ws; pend.split_k = p.split_k; pend.M = M; pend.N = w->N; pend.Npad = w->Npad;
            pend.bias = p.bias; pend.rowvec = p.rowvec; pend.ldrv = g.rowvec ? (g.ldrv ? g.ldrv : w->N) : 0;
            pend.rowvec_step = p.rowvec_step; pend.rowvec_step_stride = p.rowvec_step_stride;
            pend.rowvec_step_count = p.rowvec_step_count; pend.step_error = p.step_error;
            pend.residual = p.residual; pend.ldr = p.ldr;
            pend.pre_out = out; pend.store_pre = g.defer == 1;
            pend_out = out;
        }
        chk(pcdm_gemm(&p, st), "pcdm_gemm");
    }
    // should the producer of this LayerNorm -> Linear pair's rows write partials?  (pcdms_amd.ops.ln_wants_row_stats with a tuned table)
    bool ln_wants_stats(int M, const PW* w, const PW* w_ln, int epilogue) const {
        if (!w || !w_ln || !w_ln->wsum || w->K == 320 || w->K % 64 || w->K > 1280 || getenv_off("PCDM_LN_TILED")) return false;
        auto it = u->tiles.find(TileKey{1, M, w->Npad, w->K, 0, 0, 0, epilogue, 0, 0, 0});
        return it != u->tiles.end() && it->second.first > 0 && it->second.second == 2;
    }
    // LayerNorm -> GEMM: the folded form on the A-in-registers kernel when the table says so, two launches otherwise
    void gemm_ln(const void* a, int64_t lda, int M, const PW* w, const PW* w_ln, const float* gamma, const float* beta, float eps, void* ln_buf,
                 void* out, G g) {
        if (rc || !w) return;
        if (w_ln && w_ln->wsum && (w->K == 320 || !getenv_off("PCDM_LN_TILED"))) {   // (PCDM_LN_TILED=0: levels 1-3 keep their LayerNorm launches: A/B)
            auto it = u->tiles.find(TileKey{1, M, w->Npad, w->K, 0, 0, 0, g.epilogue, 0, 0, 0});
            if (it != u->tiles.end() && it->second.first > 0) {   // (0 = LayerNorm launch + plain GEMM; 31.. rowgemm.hip; else an LNF instance of gemm.hip)
                pcdm_gemm_params p;
                memset(&p, 0, sizeof(p));
        p.struct_size = (uint32_t)sizeof(p);
                p.a = a; p.lda = lda; p.c1 = w->K;
                p.w = w_ln->w; p.M = M; p.N = w_ln->N; p.K = w_ln->K; p.Npad = w_ln->Npad;
                p.bias = w_ln->bias;
                p.rows_per_batch = g.rows_per_batch ? g.rows_per_batch : M;
                p.epilogue = g.epilogue; p.vt_col0 = g.vt_col0;
                p.out = out; p.ldo = g.ldo ? g.ldo : w->N;
                p.out2 = g.out2; p.ldo2 = g.ldo2;
                p.ln_wsum = w_ln->wsum; p.ln_eps = eps;
                if (it->second.second == 2 && g.row_stats && stats_valid) p.ln_row_stats = g.row_stats;   // (mode 2: merge the producer's partials)
                p.tile = it->second.first;
                const int rc_ = pcdm_gemm(&p, st);
                if (rc_ != -1) {   // (-1: refused before any launch -- e.g. 88 tokens per image for the V^T pass of a key tuned at 352: two launches,
                    chk(rc_, "pcdm_gemm (LayerNorm folded)");   //  as pcdms_amd.ops._gemm_ln does)
                    return;
                }
            }
        }
        chk(pcdm_layernorm(a, ln_buf, M, w->K, eps, gamma, beta, st), "pcdm_layernorm");
        g.row_stats = nullptr;   // (here it meant the CONSUMER's partials; gemm() would read it as a producer request -- pcdms_amd.ops' two_launches() passes none)
        gemm(ln_buf, w->K, M, w, out, g);
    }
    void groupnorm(const void* x1, int C1, const void* x2, int C2, int B, int HW, float eps, const float* gamma, const float* beta, int silu, void* y) {
        if (rc) return;
        if (pend_out) {
            if (pend_out != x1 || pend.N != C1) { rc = -1; u->err = "deferred split-K reduce: the next GroupNorm reads another tensor"; return; }
            pend_out = nullptr;
            chk(pcdm_groupnorm_splitk(&pend, x2, C2, B, HW, u->cfg.norm_groups, eps, gamma, beta, silu, y, buf<float>("gnws"), st), "pcdm_groupnorm_splitk");
            return;
        }
        chk(pcdm_groupnorm(x1, C1, x2, C2, B, HW, u->cfg.norm_groups, eps, gamma, beta, silu, y, buf<float>("gnws"), st), "pcdm_groupnorm");
    }
};

int64_t lp8(int64_t v) { return (v + 7) / 8 * 8; }
int64_t lp16(int64_t v) { return (v + 15) / 16 * 16; }

bool has_cross(const pcdm_unet_config& c, int level) { return c.cross_attn[level] != 0; }

// transformer prefixes in registration / schedule order with (channels, heads)
std::vector<std::tuple<std::string, int, int>> transformers(const pcdm_unet_config& c) {
    std::vector<std::tuple<std::string, int, int>> t;
    const int n = c.n_levels, L = c.layers_per_block;
    for (int i = 0; i < n; ++i)
        if (has_cross(c, i))
            for (int j = 0; j < L; ++j) t.emplace_back("down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j) + ".", c.block_out_channels[i], c.heads[i]);
    t.emplace_back("mid_block.attentions.0.", c.block_out_channels[n - 1], c.heads[n - 1]);
    for (int i = 0; i < n; ++i)
        if (has_cross(c, n - 1 - i))
            for (int j = 0; j < L + 1; ++j)
                t.emplace_back("up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j) + ".", c.block_out_channels[n - 1 - i], c.heads[n - 1 - i]);
    return t;
}

int make_plan(pcdm_unet* u, int B, int h, int w, int L) {
    const auto key = std::make_tuple(B, h, w, L, g_redzone, (int)u->freeu);
    if (u->plan_key == key && !u->bufs.empty()) return 0;
    const pcdm_unet_config& c = u->cfg;
    u->bufs.clear();
    u->order.clear();
    Planner P{u};
    const int n = c.n_levels;
    const int C0 = c.block_out_channels[0], temb_dim = 4 * C0;
    int Cmax = 0;
    for (int i = 0; i < n; ++i) Cmax = c.block_out_channels[i] > Cmax ? c.block_out_channels[i] : Cmax;
    const int64_t HW = (int64_t)h * w, M0 = B * HW;
    int temb_n = 0;
    temb_offsets(c, &temb_n);
    // ---- conditioning (step-invariant)
    P.add("gnws", pcdm_groupnorm_ws_floats(B, 4096) * 4);
    P.add("splitk", kSplitKFloats * 4);
    P.add("cls1", (int64_t)B * temb_dim * 4);
    P.add("cls2", (int64_t)B * temb_dim * 4);
    P.add("pose", M0 * C0 * 2);
    P.add("ctx", (int64_t)B * L * c.cross_attention_dim * 2);
    for (auto& t : transformers(c)) {
        const int cc = std::get<1>(t);
        P.add("k2:" + std::get<0>(t), (int64_t)B * L * cc * 2);
        P.add("vt2:" + std::get<0>(t), (int64_t)B * cc * lp8(L) * 2);
        // e4m3 copies of the context K / V^T (1 byte per element; key axis padded to 16); laid out whether or not fp8 is switched on, so
        // that switching does not move the other buffers (a captured graph stays valid)
        P.add("k2_8:" + std::get<0>(t), (int64_t)B * L * cc);
        P.add("vt2_8:" + std::get<0>(t), (int64_t)B * cc * lp16(L));
    }
    // ---- per step
    P.add("t_emb", (int64_t)B * C0 * 4);
    P.add("e1", (int64_t)B * temb_dim * 4);
    P.add("emb", (int64_t)B * temb_dim * 4);
    P.add("emb_bf", (int64_t)B * temb_dim * 2);
    P.add("temb", (int64_t)B * temb_n * 4);
    // activations: sized for level 0 (the largest at every name); channel maxima from the topology
    int cin_max = 0;
    for (auto& r : resnets(c)) cin_max = std::get<1>(r) > cin_max ? std::get<1>(r) : cin_max;
    // rows x channels never exceed M0 x max(channels at that level): a safe bound is max over levels of M_l * C_l-ish; use per-level maxima
    int64_t act = 0, act_gn = 0, act_ff = 0, act_qk = 0, act_vt = 0, act_vt8 = 0;
    {
        int hh = h, ww = w;
        for (int i = 0; i < n; ++i) {
            const int64_t M = (int64_t)B * hh * ww;
            const int ci = c.block_out_channels[i];
            int cin_l = ci;
            for (auto& r : resnets(c))
                if (std::get<3>(r) == i) cin_l = std::get<1>(r) > cin_l ? std::get<1>(r) : cin_l;
            // the upsampling conv of up-block (n-1-i-1 .. ) writes level i rows with the channels of level i+1
            const int cup = i + 1 < n ? c.block_out_channels[i + 1] : ci;
            act = std::max(act, M * std::max(ci, cup) * 2);
            act_gn = std::max(act_gn, M * cin_l * 2);
            act_ff = std::max(act_ff, M * 4 * ci * 2);
            act_qk = std::max(act_qk, M * 2 * ci * 2);
            act_vt = std::max(act_vt, (int64_t)B * ci * lp8((int64_t)hh * ww) * 2);
            act_vt8 = std::max(act_vt8, (int64_t)B * ci * lp16((int64_t)hh * ww));
            if (i != n - 1) { hh = (hh - 1) / 2 + 1; ww = (ww - 1) / 2 + 1; }
        }
    }
    for (const char* nm : {"r", "rb", "u", "ub", "r2", "c1", "sc", "t0", "t1", "ln", "q2", "at", "us"}) P.add(nm, act);
    P.add("step_err", kAlign);       // int32: a forward found the device step counter outside the time table (pcdm_unet_step_overflow)
    P.add("rs", act / 8 + kAlign);   // LayerNorm partials: [M][C / 32][2] fp32 = an eighth of an activation's bytes
    P.add("gn", act_gn);
    P.add("ff", act_ff);
    P.add("qk", act_qk);
    P.add("vt", act_vt);
    P.add("k8", act_qk / 4);        // e4m3 K of the self-attention in flight: M x C bytes (act_qk = M x 2C x 2 bytes)
    P.add("vt8", act_vt8);
    {   // skip tensors: one buffer per skip, exact sizes
        int hh = h, ww = w;
        P.add("skip0", M0 * C0 * 2);
        for (int i = 0; i < n; ++i) {
            const int64_t M = (int64_t)B * hh * ww;
            for (int j = 0; j < c.layers_per_block; ++j) P.add("d" + std::to_string(i) + "." + std::to_string(j), M * c.block_out_channels[i] * 2);
            if (i != n - 1) {
                hh = (hh - 1) / 2 + 1; ww = (ww - 1) / 2 + 1;
                P.add("ds" + std::to_string(i), (int64_t)B * hh * ww * c.block_out_channels[i] * 2);
            }
        }
    }
    if (u->freeu) {   // FreeU (pcdm_unet_set_freeu): the filtered skip of the resnet in flight and, for planes beyond the one-launch size, the coefficients
        int64_t fs = 0, fw = 0;
        std::vector<std::pair<int, int>> hw{{h, w}};
        for (int i = 1; i < n; ++i) hw.emplace_back((hw.back().first - 1) / 2 + 1, (hw.back().second - 1) / 2 + 1);
        for (int i = 0; i < n && i < 2; ++i) {
            const int lv = n - 1 - i, out = c.block_out_channels[lv], inc = c.block_out_channels[lv > 0 ? lv - 1 : 0];
            const int cs = std::max(out, inc), hh = hw[lv].first, ww = hw[lv].second;
            fs = std::max(fs, (int64_t)B * hh * ww * cs * 2);
            fw = std::max(fw, pcdm_freeu_ws_bytes(B, hh, ww, 8, cs));
        }
        P.add("fu_s", fs);
        if (fw > 0) P.add("fu_ws", fw);
    }
    {   // the live regions in offset order (a name laid out twice keeps its last region only: Planner::add)
        std::vector<std::string> live;
        for (auto it = u->order.rbegin(); it != u->order.rend(); ++it)
            if (std::find(live.begin(), live.end(), *it) == live.end()) live.push_back(*it);
        std::sort(live.begin(), live.end(), [&](const std::string& a, const std::string& b) { return u->bufs[a].off < u->bufs[b].off; });
        u->order.swap(live);
    }
    u->ws_bytes = P.off;
    u->plan_key = key;
    return 0;
}
}  // namespace

extern "C" int pcdm_set_workspace_redzone(int64_t bytes) {
    if (bytes < 0 || bytes % kAlign) return -1;
    g_redzone = bytes;
    return 0;
}

extern "C" int64_t pcdm_get_workspace_redzone(void) { return g_redzone; }

extern "C" pcdm_unet* pcdm_unet_create(const pcdm_unet_config* cfg) {
    if (!cfg || cfg->n_levels < 1 || cfg->n_levels > 8 || cfg->layers_per_block < 1) return nullptr;
    for (int i = 0; i < cfg->n_levels; ++i)
        if (cfg->block_out_channels[i] % 64 || cfg->heads[i] <= 0 || cfg->block_out_channels[i] / cfg->heads[i] != 64) return nullptr;
    pcdm_unet* u = new pcdm_unet();
    u->cfg = *cfg;
    // the committed tuning table (pcdms_amd/tuning/gfx950.json, measured on MI355X by tools/tune_gemm_shapes.py) is compiled in: a host
    // without the Python tuner runs on the measured (tile, split-K) set from the start; pcdm_unet_set_tile overrides single entries
    static const int kTable[][13] = {
#include "tuning_table.inc"
    };
    // ... on the architecture it was measured on only: any other device starts on pcdm_gemm's static heuristic
    bool gfx950 = true;
#ifndef PCDM_EMU
    {
        int dev = 0;
        hipDeviceProp_t prop;
        gfx950 = hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0;
    }
#endif
    if (gfx950)
        for (const auto& r : kTable) u->tiles[TileKey{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10]}] = {r[11], r[12]};
    return u;
}

extern "C" void pcdm_unet_destroy(pcdm_unet* u) { delete u; }

extern "C" const char* pcdm_unet_last_error(const pcdm_unet* u) { return u ? u->err.c_str() : "null context"; }

extern "C" int pcdm_unet_set_weight(pcdm_unet* u, const char* name, const void* w, const float* bias, const float* wsum, int N, int K, int Npad,
                                    int cin) {
    if (!u || !name || !w || N <= 0 || K <= 0 || Npad < N) return -1;
    PW p;
    p.w = w; p.bias = bias; p.wsum = wsum; p.N = N; p.K = K; p.Npad = Npad; p.cin = cin;
    u->w[name] = p;
    u->bufs.clear();
    u->cond_of_ws.clear();   // (the plan is rebuilt: buffers move)
    return 0;
}

extern "C" int pcdm_unet_set_vector(pcdm_unet* u, const char* name, const float* v, int n) {
    if (!u || !name || !v || n <= 0) return -1;
    u->v[name] = Vec{v, n};
    return 0;
}

extern "C" int pcdm_unet_set_tile(pcdm_unet* u, int ln, int M, int Npad, int K, int conv, int stride, int upsample, int epilogue, int two_source,
                                  int residual, int zero_rows, int tile, int split_k) {
    if (!u || tile < 0) return -1;
    u->tiles[TileKey{ln, M, Npad, K, conv, stride, upsample, epilogue, two_source, residual, zero_rows}] = {tile, split_k};
    return 0;
}

// Every attention of the UNet (self and cross) with e4m3 operands on the MX-scaled fp8 MFMA (BASELINE.json configs[4]; pcdms_amd's
// set_attention_precision("fp8")).  Switch BEFORE pcdm_unet_prepare_conditioning (which quantises the context K / V^T) and before capturing.
extern "C" int pcdm_unet_set_attention_fp8(pcdm_unet* u, int on) {
    if (!u) return -1;
    if ((on != 0) != u->attn_fp8) u->cond_of_ws.clear();   // (outstanding conditionings lack / carry the e4m3 copies)
    u->attn_fp8 = on != 0;
    return 0;
}

extern "C" int pcdm_unet_set_freeu(pcdm_unet* u, int on, float s1, float s2, float b1, float b2) {
    if (!u) return -1;
    if ((on != 0) != u->freeu) {   // (the plan gains / loses the FreeU buffers: every buffer moves)
        u->bufs.clear();
        u->cond_of_ws.clear();
    }
    u->freeu = on != 0;
    u->fu_s[0] = s1; u->fu_s[1] = s2; u->fu_b[0] = b1; u->fu_b[1] = b2;
    return 0;
}

extern "C" int pcdm_unet_get_tile(const pcdm_unet* u, int ln, int M, int Npad, int K, int conv, int stride, int upsample, int epilogue, int two_source,
                                  int residual, int flag, int* tile, int* split_k) {
    if (!u) return -1;
    auto it = u->tiles.find(TileKey{ln, M, Npad, K, conv, stride, upsample, epilogue, two_source, residual, flag});
    if (it == u->tiles.end()) return -1;
    if (tile) *tile = it->second.first;
    if (split_k) *split_k = it->second.second;
    return 0;
}

extern "C" int64_t pcdm_unet_workspace_bytes(pcdm_unet* u, int B, int h, int w, int L) {
    if (!u || B <= 0 || h <= 0 || w <= 0 || L <= 0) return -1;
    if (make_plan(u, B, h, w, L)) return -1;
    return u->ws_bytes;
}

extern "C" int pcdm_unet_workspace_layout(pcdm_unet* u, int B, int h, int w, int L, int index, const char** name, int64_t* offset, int64_t* bytes) {
    if (!u || B <= 0 || h <= 0 || w <= 0 || L <= 0 || make_plan(u, B, h, w, L)) return -1;
    const int n = (int)u->order.size();
    if (index == -1) return n;
    if (index < 0 || index >= n) return -1;
    const auto it = u->bufs.find(u->order[index]);
    if (name) *name = it->first.c_str();
    if (offset) *offset = it->second.off;
    if (bytes) *bytes = it->second.bytes;
    return n;
}

// Zero the regions that must start at zero (GroupNorm arrival counters, the padding columns of the V^T buffers); once per workspace.
extern "C" int pcdm_unet_workspace_init(pcdm_unet* u, int B, int h, int w, int L, void* workspace, pcdm_stream_t s) {
    if (!u || !workspace || make_plan(u, B, h, w, L)) return -1;
#ifdef PCDM_EMU
    memset(workspace, 0, (size_t)u->ws_bytes);
    (void)s;
    return 0;
#else
    return hipMemsetAsync(workspace, 0, (size_t)u->ws_bytes, (hipStream_t)s) == hipSuccess ? 0 : -1000;
#endif
}

// Step-invariant part of a sampling call (pcdms_amd/unet.py::prepare_conditioning; ref :688-708, :742 and the 16 attn2.to_k / to_v):
// class embedding, NHWC bf16 pose feature, cross-attention K / V^T of the context.  ehs fp32 [B, L, ctx] (device); class_labels fp32
// [B, class_embed_dim] or NULL; pose fp32 NCHW [pose_b, C0, h, w] (pose_b = 1 or B) or NULL; the first zero_ctx_batches batch entries of
// ehs are all-zero (their K / V are not projected, their cross-attention is not run).
extern "C" int pcdm_unet_prepare_conditioning(pcdm_unet* u, int B, int h, int w, int L, const float* ehs, const float* class_labels, const float* pose,
                                              int pose_b, int zero_ctx_batches, void* workspace, pcdm_stream_t s) {
    if (!u || !ehs || !workspace || make_plan(u, B, h, w, L)) return -1;
    const pcdm_unet_config& c = u->cfg;
    Run R{u, (char*)workspace, s};
    const int temb_dim = 4 * c.block_out_channels[0];
    int n0 = zero_ctx_batches;
    if (n0 < 0 || n0 > B) return -1;
    if (n0 == B) n0 = B > 1 ? B - 1 : 0;
    pcdm_unet::WsCond wc;
    wc.B = B; wc.h = h; wc.w = w; wc.L = L; wc.n0 = n0; wc.pose_b = pose ? pose_b : 0;
    u->cond_of_ws[workspace] = wc;   // (also drops a time table prepared for the previous conditioning: the class embedding changed)
    if (c.class_embed) {
        if (!class_labels) return -1;
        const PW *c1 = R.pw("class_embedding.linear_1"), *c2 = R.pw("class_embedding.linear_2");
        if (R.rc) return R.rc;
        R.chk(pcdm_small_linear(class_labels, c1->w, c1->bias, nullptr, R.buf<float>("cls1"), B, c1->K, c1->N, 0, 1, s), "pcdm_small_linear");
        R.chk(pcdm_small_linear(R.buf<float>("cls1"), c2->w, c2->bias, nullptr, R.buf<float>("cls2"), B, c2->K, c2->N, 0, 0, s), "pcdm_small_linear");
    }
    if (pose) {
        if (pose_b != 1 && pose_b != B) return -1;
        // one NHWC copy per batch entry, also for a batch-1 pose feature: conv_in then adds it as a plain residual (res_mod = M: the
        // 16-byte-per-lane epilogue; a broadcast residual takes the per-element one)
        const int C0p = c.block_out_channels[0];
        if (pose_b == B) R.chk(pcdm_nchw_f32_to_nhwc_bf16(pose, R.buf("pose"), B, C0p, C0p, h * w, s), "nchw_to_nhwc");
        else
            for (int b = 0; b < B; ++b)
                R.chk(pcdm_nchw_f32_to_nhwc_bf16(pose, R.buf<char>("pose") + (int64_t)b * h * w * C0p * 2, 1, C0p, C0p, h * w, s), "nchw_to_nhwc");
    }
    (void)temb_dim;
    const int Bc = B - n0;
    R.chk(pcdm_f32_to_bf16(ehs + (int64_t)n0 * L * c.cross_attention_dim, R.buf("ctx"), (int64_t)Bc * L * c.cross_attention_dim, s), "f32_to_bf16");
    for (auto& t : transformers(c)) {
        const std::string& p = std::get<0>(t);
        const int cc = std::get<1>(t);
        Run::G g;
        g.rows_per_batch = L;
        g.epilogue = PCDM_EPI_SPLIT_VT;
        g.out2 = R.buf("vt2:" + p);
        g.ldo2 = lp8(L);
        g.vt_col0 = cc;
        g.ldo = cc;
        R.gemm(R.buf("ctx"), c.cross_attention_dim, Bc * L, R.pw(p + "kv2"), R.buf("k2:" + p), g);
        if (u->attn_fp8 && !R.rc) {   // e4m3 copies, once per sampling call (pcdms_amd/unet.py::prepare_conditioning)
            R.chk(pcdm_quantize_fp8(R.buf("k2:" + p), R.buf("k2_8:" + p), (int64_t)Bc * L, cc, cc, cc, cc, 1.0f, s), "pcdm_quantize_fp8");
            R.chk(pcdm_quantize_fp8(R.buf("vt2:" + p), R.buf("vt2_8:" + p), (int64_t)Bc * cc, L, (int)lp16(L), lp8(L), lp16(L), 1.0f, s), "pcdm_quantize_fp8");
        }
    }
    return R.rc;
}

// The caller guarantees that, on this workspace, batch entries b and b + B/2 always carry the same x_in rows and the same pose feature (the
// two classifier-free-guidance halves): conv_in, the first norm1 and the first conv1's contraction then run once for both
// (pcdm_gemm_params.dup_rows).  Call after pcdm_unet_prepare_conditioning (which resets it to 0).
extern "C" int pcdm_unet_set_shared_cfg_input(pcdm_unet* u, void* workspace, int shared) {
    if (!u) return -1;
    auto it = u->cond_of_ws.find(workspace);
    if (it == u->cond_of_ws.end()) return -1;
    if (shared && (it->second.B % 2 || getenv_off("PCDM_SHARE_CFG_PREFIX"))) shared = 0;
    it->second.shared = shared ? 1 : 0;
    return 0;
}

// The time / class embedding MLPs and every ResnetBlock2D.time_emb_proj for ALL steps of a timestep table (they depend on the timestep and
// the class labels only): once per sampling call, after pcdm_unet_prepare_conditioning on the same workspace, instead of five launches
// per denoise step.  `table` is caller-owned device memory of pcdm_unet_time_table_bytes(u, n, B) bytes (the table proper, then the
// scratch of this call); pcdm_unet_forward calls on this workspace that pass the SAME t_dev together with a device step counter then pick
// their block by that counter (pcdm_gemm_params.rowvec_step).  Same per-row arithmetic as the per-step launches: bit-identical.
extern "C" int64_t pcdm_unet_time_table_bytes(const pcdm_unet* u, int n, int B) {
    if (!u || n <= 0 || B <= 0) return -1;
    int temb_n = 0;
    temb_offsets(u->cfg, &temb_n);
    const int64_t C0 = u->cfg.block_out_channels[0], D = 4 * C0;
    return round_up((int64_t)n * B * temb_n * 4, kAlign) + round_up((int64_t)n * C0 * 4, kAlign) + 2 * round_up((int64_t)n * D * 4, kAlign) +
           round_up((int64_t)n * B * D * 2, kAlign);
}

static int prepare_timesteps_impl(pcdm_unet* u, const void* t_dev, bool t_f32, int n, void* table, void* workspace, pcdm_stream_t s) {
    if (!u || !t_dev || n <= 0 || !table || !workspace) return -1;
    auto it = u->cond_of_ws.find(workspace);
    if (it == u->cond_of_ws.end()) { u->err = "pcdm_unet_prepare_conditioning has not run on this workspace"; return -1; }
    if (getenv_off("PCDM_TIME_TABLE")) return 0;
    const pcdm_unet_config& c = u->cfg;
    const int B = it->second.B;
    if (make_plan(u, B, it->second.h, it->second.w, it->second.L)) return -1;
    Run R{u, (char*)workspace, s};
    int temb_n = 0;
    temb_offsets(c, &temb_n);
    const int64_t C0 = c.block_out_channels[0], D = 4 * C0;
    char* base = (char*)table;
    float* tab = (float*)base;                      base += round_up((int64_t)n * B * temb_n * 4, kAlign);
    float* t_emb = (float*)base;                    base += round_up((int64_t)n * C0 * 4, kAlign);
    float* e1 = (float*)base;                       base += round_up((int64_t)n * D * 4, kAlign);
    float* emb_t = (float*)base;                    base += round_up((int64_t)n * D * 4, kAlign);
    void* emb_bf = base;
    const PW *t1 = R.pw("time_embedding.linear_1"), *t2 = R.pw("time_embedding.linear_2"), *tp = R.pw("time_emb_proj");
    if (R.rc) return R.rc;
    R.chk(t_f32 ? pcdm_timestep_embedding_rows_f32((const float*)t_dev, n, t_emb, (int)C0, c.flip_sin_to_cos, c.freq_shift, s)
                : pcdm_timestep_embedding_rows((const int64_t*)t_dev, n, t_emb, (int)C0, c.flip_sin_to_cos, c.freq_shift, s), "pcdm_timestep_embedding_rows");
    for (int r0 = 0; r0 < n; r0 += 32) {   // (pcdm_small_linear takes <= 32 rows; rows are independent)
        const int nr = n - r0 < 32 ? n - r0 : 32;
        R.chk(pcdm_small_linear(t_emb + (int64_t)r0 * C0, t1->w, t1->bias, nullptr, e1 + (int64_t)r0 * D, nr, t1->K, t1->N, 0, 1, s), "pcdm_small_linear");
        R.chk(pcdm_small_linear(e1 + (int64_t)r0 * D, t2->w, t2->bias, nullptr, emb_t + (int64_t)r0 * D, nr, t2->K, t2->N, 0, 0, s), "pcdm_small_linear");
    }
    R.chk(pcdm_time_class_combine(emb_t, c.class_embed ? R.buf<float>("cls2") : nullptr, emb_bf, n, B, (int)D, s), "pcdm_time_class_combine");
    {   // the SAME tile as the per-step launch (M = B rows): identical bits
        pcdm_gemm_params p;
        memset(&p, 0, sizeof(p));
        p.struct_size = (uint32_t)sizeof(p);
        p.a = emb_bf; p.lda = D; p.c1 = tp->K;
        p.w = tp->w; p.M = n * B; p.N = tp->N; p.K = tp->K; p.Npad = tp->Npad;
        p.bias = tp->bias;
        p.rows_per_batch = 1;
        p.epilogue = PCDM_EPI_NCHW_F32;
        p.out = tab; p.ldo = tp->N;
        auto tk = u->tiles.find(TileKey{0, B, tp->Npad, tp->K, 0, 0, 0, PCDM_EPI_NCHW_F32, 0, 0, 0});
        p.tile = (tk != u->tiles.end() && tk->second.second <= 1) ? tk->second.first : 8;
        R.chk(pcdm_gemm(&p, s), "pcdm_gemm (time_emb_proj table)");
    }
    if (R.rc) return R.rc;
    it->second.time_table = tab;
    it->second.time_steps = n;
    it->second.time_t_dev = t_dev;
#ifdef PCDM_EMU
    *R.buf<int32_t>("step_err") = 0;
#else
    if (hipMemsetAsync(R.buf<int32_t>("step_err"), 0, sizeof(int32_t), (hipStream_t)s) != hipSuccess) return -1000;
#endif
    return 0;
}

extern "C" int pcdm_unet_prepare_timesteps(pcdm_unet* u, const int64_t* t_dev, int n, void* table, void* workspace, pcdm_stream_t s) {
    return prepare_timesteps_impl(u, t_dev, false, n, table, workspace, s);
}
extern "C" int pcdm_unet_prepare_timesteps_f32(pcdm_unet* u, const float* t_dev, int n, void* table, void* workspace, pcdm_stream_t s) {
    return prepare_timesteps_impl(u, t_dev, true, n, table, workspace, s);
}

// Has a forward on this workspace read the time table with a device step counter outside [0, n)?  (the consumers clamp it and raise this flag:
// pcdm_gemm_params.rowvec_step_count / step_error).  Synchronous 4-byte read behind everything enqueued on s.
extern "C" int pcdm_unet_step_overflow(pcdm_unet* u, void* workspace, int* flag_out, pcdm_stream_t s) {
    if (!u || !workspace || !flag_out) return -1;
    const auto cit = u->cond_of_ws.find(workspace);
    if (cit == u->cond_of_ws.end()) { u->err = "pcdm_unet_prepare_conditioning has not run on this workspace"; return -1; }
    if (make_plan(u, cit->second.B, cit->second.h, cit->second.w, cit->second.L)) return -1;
    Run R{u, (char*)workspace, s};
    int32_t v = 0;
#ifdef PCDM_EMU
    v = *R.buf<int32_t>("step_err");
#else
    if (hipMemcpyAsync(&v, R.buf<int32_t>("step_err"), sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)s) != hipSuccess) return -1000;
    if (hipStreamSynchronize((hipStream_t)s) != hipSuccess) return -1000;
#endif
    *flag_out = v != 0;
    return 0;
}

// One UNet forward (pcdms_amd/unet.py::_forward_nhwc): x_in NHWC bf16 [B, h, w, conv_in.cin]; the timestep is t_dev[step_dev ? *step_dev : 0]
// (device memory: graph-replayable); eps_out fp32 NCHW [B, out_channels, h, w].  prepare_conditioning must have run on this workspace.
// (t_f32: t_dev is a float table -- pcdm_unet_forward_f32 -- else int64)
static int unet_forward_impl(pcdm_unet* u, const void* x_in, const void* t_dev, bool t_f32, const int32_t* step_dev, int B, int h, int w, int L,
                             int pose_b, void* workspace, float* eps_out, pcdm_stream_t s) {
    if (!u || !x_in || !t_dev || !workspace || !eps_out || make_plan(u, B, h, w, L)) return -1;
    const pcdm_unet_config& c = u->cfg;
    Run R{u, (char*)workspace, s};
    const int n = c.n_levels, Lb = c.layers_per_block, G = c.norm_groups;
    const int C0 = c.block_out_channels[0], temb_dim = 4 * C0;
    const float eps = c.norm_eps;
    int temb_n = 0;
    const std::map<std::string, int> toff = temb_offsets(c, &temb_n);
    const auto cit = u->cond_of_ws.find(workspace);
    if (cit == u->cond_of_ws.end() || cit->second.B != B || cit->second.h != h || cit->second.w != w || cit->second.L != L || cit->second.pose_b != pose_b) {
        u->err = cit == u->cond_of_ws.end() ? "pcdm_unet_prepare_conditioning has not run on this workspace"
                                            : "this workspace's conditioning was prepared for another shape / pose_b";
        return -1;
    }
    const int n0 = cit->second.n0;
    const bool shared = cit->second.shared != 0;   // the CFG halves share conv_in / the first norm1 / the first conv1's contraction

    // ---- 1. time / class embedding (ref :661-708): from the per-call table when one was prepared for this timestep table, else five launches
    const bool use_table = cit->second.time_table && step_dev && cit->second.time_t_dev == t_dev;
    const int32_t* rv_step = use_table ? step_dev : nullptr;
    const int64_t rv_stride = use_table ? (int64_t)B * temb_n : 0;
    const int rv_count = use_table ? cit->second.time_steps : 0;          // the step counter is bounded into the table on the device (ABI 4)
    int32_t* rv_err = use_table ? R.buf<int32_t>("step_err") : nullptr;
    if (!use_table) {
        // the length of t_dev this path knows: 1 without a counter; with a counter and no table prepared for this t_dev the caller's contract
        // (counter < length of t_dev) is all there is -- INT32_MAX leaves the counter as it is, a negative one reads row 0 (include/pcdm.h)
        const int t_rows = step_dev ? INT32_MAX : 1;
        R.chk(t_f32 ? pcdm_timestep_embedding_f32((const float*)t_dev, t_rows, step_dev, nullptr, R.buf<float>("t_emb"), B, C0, c.flip_sin_to_cos, c.freq_shift, s)
                    : pcdm_timestep_embedding((const int64_t*)t_dev, t_rows, step_dev, nullptr, R.buf<float>("t_emb"), B, C0, c.flip_sin_to_cos, c.freq_shift, s),
              "pcdm_timestep_embedding");
        const PW *t1 = R.pw("time_embedding.linear_1"), *t2 = R.pw("time_embedding.linear_2");
        if (R.rc) return R.rc;
        R.chk(pcdm_small_linear(R.buf<float>("t_emb"), t1->w, t1->bias, nullptr, R.buf<float>("e1"), B, t1->K, t1->N, 0, 1, s), "pcdm_small_linear");
        // emb = time_emb + class_emb is only ever consumed as silu(emb) (ResnetBlock2D): applied here, once
        R.chk(pcdm_small_linear(R.buf<float>("e1"), t2->w, t2->bias, c.class_embed ? R.buf<float>("cls2") : nullptr, R.buf<float>("emb"), B, t2->K, t2->N, 0,
                                c.class_embed ? 2 : 1, s), "pcdm_small_linear");
        R.chk(pcdm_f32_to_bf16(R.buf<float>("emb"), R.buf("emb_bf"), (int64_t)B * temb_dim, s), "f32_to_bf16");
        Run::G g;
        g.rows_per_batch = 1;
        g.epilogue = PCDM_EPI_NCHW_F32;
        R.gemm(R.buf("emb_bf"), temb_dim, B, R.pw("time_emb_proj"), R.buf("temb"), g);   // every ResnetBlock2D.time_emb_proj in one launch
    }
    const float* temb = use_table ? cit->second.time_table : R.buf<float>("temb");

    auto chk_gn_half = [&](const void* x1, int C1, int Bs, int HW_, float e, const float* gamma, const float* beta) {
        R.groupnorm(x1, C1, nullptr, 0, Bs, HW_, e, gamma, beta, 1, R.buf("gn"));
    };
    auto resnet = [&](const std::string& p, const void* x1, int C1, const void* x2, int C2, int HW_, int hh, int ww, const std::string& out_name,
                      bool gn_next, bool shared_in = false) -> void* {   // gn_next: the next reader of the block's output is a GroupNorm (split-K reduce folded into it)
        const bool composed = u->w.count(p + "conv2s") != 0;   // conv2 + conv_shortcut registered as one set of rows (then neither need be registered)
        const PW *cv1 = R.pw(p + "conv1"), *cv2 = composed ? nullptr : R.pw(p + "conv2");
        if (R.rc) return nullptr;
        const int cin = C1 + C2, cout = cv1->N, M = B * HW_;
        Run::G g;
        g.conv = 1; g.B = B; g.Hi = hh; g.Wi = ww; g.Ho = hh; g.Wo = ww;
        g.rowvec = temb + toff.at(p); g.ldrv = temb_n; g.rows_per_batch = HW_;
        g.rowvec_step = rv_step; g.rowvec_step_stride = rv_stride;
        g.rowvec_step_count = rv_count; g.step_error = rv_err;
        if (shared_in) {   // the CFG halves still have the same x1: norm1 and conv1's contraction once, two epilogues
            const int Bs = B / 2, Ms = Bs * HW_;
            chk_gn_half(x1, C1, Bs, HW_, eps, R.vec(p + "norm1.weight"), R.vec(p + "norm1.bias"));
            g.B = Bs; g.dup_rows = Ms;
            R.gemm(R.buf("gn"), cin, Ms, cv1, R.buf("c1"), g);
        } else {
            R.groupnorm(x1, C1, x2, C2, B, HW_, eps, R.vec(p + "norm1.weight"), R.vec(p + "norm1.bias"), 1, R.buf("gn"));
            g.defer = 2;
            R.gemm(R.buf("gn"), cin, M, cv1, R.buf("c1"), g);
        }
        R.groupnorm(R.buf("c1"), cout, nullptr, 0, B, HW_, eps, R.vec(p + "norm2.weight"), R.vec(p + "norm2.bias"), 1, R.buf("gn"));
        if (composed) {
            // conv2 + conv_shortcut as ONE contraction (weight rows [9 cout taps | C1 | C2], composed by the host: pcdms_amd/unet.py FUSE_SHORTCUT;
            // registered as "<resnet>conv2s"): the block's input enters through the extra K, no shortcut launch, no residual
            Run::G g2;
            g2.conv = 1; g2.B = B; g2.Hi = hh; g2.Wi = ww; g2.Ho = hh; g2.Wo = ww;
            g2.a2 = x1; g2.lda2 = C1; g2.c1 = C1;
            if (x2) { g2.a3 = x2; g2.lda3 = C2; }
            g2.rows_per_batch = HW_;
            g2.defer = gn_next ? 1 : 0;
            void* out = R.buf(out_name);
            R.gemm(R.buf("gn"), cout, M, R.pw(p + "conv2s"), out, g2);
            return out;
        }
        const void* res = x1;
        if (u->w.count(p + "conv_shortcut")) {
            Run::G gs;
            gs.a2 = x2; gs.lda2 = C2;
            R.gemm(x1, C1, M, R.pw(p + "conv_shortcut"), R.buf("sc"), gs);
            res = R.buf("sc");
        }
        Run::G g2;
        g2.conv = 1; g2.B = B; g2.Hi = hh; g2.Wi = ww; g2.Ho = hh; g2.Wo = ww;
        g2.residual = res; g2.ldr = cout; g2.res_mod = M;
        g2.rows_per_batch = HW_;
        g2.defer = gn_next ? 1 : 0;
        void* out = R.buf(out_name);
        R.gemm(R.buf("gn"), cout, M, cv2, out, g2);
        return out;
    };

    auto transformer = [&](const std::string& p, const void* x, int cc, int H, int HW_, const std::string& out_name) -> void* {
        const int M = B * HW_;
        const std::string b = p + "transformer_blocks.0.";
        R.groupnorm(x, cc, nullptr, 0, B, HW_, 1e-6f, R.vec(p + "norm.weight"), R.vec(p + "norm.bias"), 0, R.buf("gn"));
        const int64_t r0 = (int64_t)n0 * HW_;
        float* rs = R.buf<float>("rs");            // LayerNorm partials of the rows in flight: [M][cc / 32][2] (round 5; pcdms_amd/unet.py::transformer)
        auto twin = [&](const char* nm) -> const PW* { return u->w.count(p + nm) ? &u->w[p + nm] : nullptr; };
        Run::G g0;
        if (R.ln_wants_stats(M, R.pw(p + "qkv"), twin("qkv_ln"), PCDM_EPI_SPLIT_VT)) g0.row_stats = rs;
        R.gemm(R.buf("gn"), cc, M, R.pw(p + "proj_in"), R.buf("t0"), g0);
        // self-attention
        {
            Run::G g;
            g.rows_per_batch = HW_; g.epilogue = PCDM_EPI_SPLIT_VT; g.out2 = R.buf("vt"); g.ldo2 = lp8(HW_); g.vt_col0 = 2 * cc; g.ldo = 2 * cc;
            g.row_stats = rs;
            const PW* wl = u->w.count(p + "qkv_ln") ? &u->w[p + "qkv_ln"] : nullptr;
            R.gemm_ln(R.buf("t0"), cc, M, R.pw(p + "qkv"), wl, R.vec(b + "norm1.weight"), R.vec(b + "norm1.bias"), 1e-5f, R.buf("ln"), R.buf("qk"), g);
        }
        u16* qk = R.buf<u16>("qk");
        if (R.rc) return nullptr;
        if (u->attn_fp8) {   // K and V^T quantised once per attention, Q and P inside the kernel (pcdms_amd/unet.py::transformer)
            R.chk(pcdm_quantize_fp8(qk + cc, R.buf("k8"), M, cc, cc, 2 * cc, cc, 1.0f, s), "pcdm_quantize_fp8");
            R.chk(pcdm_quantize_fp8(R.buf("vt"), R.buf("vt8"), (int64_t)B * cc, HW_, (int)lp16(HW_), lp8(HW_), lp16(HW_), 1.0f, s), "pcdm_quantize_fp8");
            R.chk(pcdm_flash_attn_fp8(qk, 2 * cc, R.buf("k8"), cc, R.buf("vt8"), lp16(HW_), R.buf("at"), cc, B, H, HW_, HW_, 0.125f, 1.0f, 1.0f, 5.0f, s),
                  "pcdm_flash_attn_fp8");
        } else
        R.chk(pcdm_flash_attn(qk, 2 * cc, qk + cc, 2 * cc, R.buf("vt"), lp8(HW_), R.buf("at"), cc, B, H, HW_, HW_, 0.125f, s), "pcdm_flash_attn");
        {
            Run::G g;
            g.residual = R.buf("t0"); g.ldr = cc; g.res_mod = M;
            if (R.ln_wants_stats(M - (int)r0, R.pw(p + "q2"), twin("q2_ln"), PCDM_EPI_STORE)) g.row_stats = rs;
            R.gemm(R.buf("at"), cc, M, R.pw(p + "o1"), R.buf("t1"), g);
        }
        // cross-attention over the context tokens; the first n0 batch entries have an all-zero context: attn2(x) == to_out.0.bias there
        u16 *t1 = R.buf<u16>("t1"), *ln = R.buf<u16>("ln"), *q2 = R.buf<u16>("q2"), *at = R.buf<u16>("at");
        {
            Run::G g;
            g.row_stats = rs + r0 * (cc / 32) * 2;
            const PW* wl = u->w.count(p + "q2_ln") ? &u->w[p + "q2_ln"] : nullptr;
            R.gemm_ln(t1 + r0 * cc, cc, M - (int)r0, R.pw(p + "q2"), wl, R.vec(b + "norm2.weight"), R.vec(b + "norm2.bias"), 1e-5f, ln + r0 * cc, q2 + r0 * cc, g);
        }
        if (R.rc) return nullptr;
        if (u->attn_fp8)
            R.chk(pcdm_flash_attn_fp8(q2 + r0 * cc, cc, R.buf("k2_8:" + p), cc, R.buf("vt2_8:" + p), lp16(L), at + r0 * cc, cc, B - n0, H, HW_, L, 0.125f, 1.0f,
                                      1.0f, 5.0f, s), "pcdm_flash_attn_fp8");
        else
        R.chk(pcdm_flash_attn(q2 + r0 * cc, cc, R.buf("k2:" + p), cc, R.buf("vt2:" + p), lp8(L), at + r0 * cc, cc, B - n0, H, HW_, L, 0.125f, s), "pcdm_flash_attn");
        {
            Run::G g;
            g.residual = t1; g.ldr = cc; g.res_mod = M; g.zero_rows = (int)r0;
            if (R.ln_wants_stats(M, R.pw(p + "ff1"), twin("ff1_ln"), PCDM_EPI_GEGLU)) g.row_stats = rs;
            R.gemm(at, cc, M, R.pw(p + "o2"), R.buf("t0"), g);
        }
        // GEGLU feed-forward
        {
            Run::G g;
            g.epilogue = PCDM_EPI_GEGLU; g.ldo = 4 * cc;
            g.row_stats = rs;
            const PW* wl = u->w.count(p + "ff1_ln") ? &u->w[p + "ff1_ln"] : nullptr;
            R.gemm_ln(R.buf("t0"), cc, M, R.pw(p + "ff1"), wl, R.vec(b + "norm3.weight"), R.vec(b + "norm3.bias"), 1e-5f, R.buf("ln"), R.buf("ff"), g);
        }
        void* out = R.buf(out_name);
        if (u->w.count(p + "ffo")) {
            // ff.net.2 (+ residual) -> proj_out (+ residual) as one two-source GEMM over [ff | t0] against [Wp W2 | Wp] (composed at load time by the
            // host: pcdms_amd/unet.py FUSE_FF_OUT; registered as "<transformer>ffo"): no launch and no M x C round trip for the state in between
            Run::G g;
            g.a2 = R.buf("t0"); g.lda2 = cc;
            g.residual = x; g.ldr = cc; g.res_mod = M;
            R.gemm(R.buf("ff"), 4 * cc, M, R.pw(p + "ffo"), out, g);
            return out;
        }
        {
            Run::G g;
            g.residual = R.buf("t0"); g.ldr = cc; g.res_mod = M;
            R.gemm(R.buf("ff"), 4 * cc, M, R.pw(p + "ff2"), R.buf("t1"), g);
        }
        Run::G g;
        g.residual = x; g.ldr = cc; g.res_mod = M;
        R.gemm(R.buf("t1"), cc, M, R.pw(p + "proj_out"), out, g);
        return out;
    };

    // ---- 2. conv_in + pose (ref :742)
    const int HW = h * w;
    struct Skip { const void* p; int hh, ww, ch; };
    std::vector<Skip> skips;
    const void* x;
    {
        Run::G g;
        g.conv = 1; g.B = B; g.Hi = h; g.Wi = w; g.Ho = h; g.Wo = w;
        if (pose_b > 0) { g.residual = R.buf("pose"); g.ldr = C0; g.res_mod = B * HW; }   // (prepare_conditioning wrote B entries)
        if (shared) {
            g.B = B / 2; g.dup_rows = (B / 2) * HW;
            if (pose_b > 0) g.res_mod = g.dup_rows;
            R.gemm(x_in, 0, (B / 2) * HW, R.pw("conv_in"), R.buf("skip0"), g);
        } else
        R.gemm(x_in, 0, B * HW, R.pw("conv_in"), R.buf("skip0"), g);
        x = R.buf("skip0");
    }
    skips.push_back({x, h, w, C0});
    // ---- 3. down (ref :746-761)
    int hh = h, ww = w;
    for (int i = 0; i < n && !R.rc; ++i) {
        const int ci = c.block_out_channels[i];
        int cprev = i == 0 ? C0 : c.block_out_channels[i - 1];
        for (int j = 0; j < Lb; ++j) {
            const std::string nm = "d" + std::to_string(i) + "." + std::to_string(j), rp = "down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j) + ".";
            if (has_cross(c, i)) {
                x = resnet(rp, x, j == 0 ? cprev : ci, nullptr, 0, hh * ww, hh, ww, "r", true, shared && i == 0 && j == 0);
                x = transformer("down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j) + ".", x, ci, c.heads[i], hh * ww, nm);
            } else {
                x = resnet(rp, x, j == 0 ? cprev : ci, nullptr, 0, hh * ww, hh, ww, nm, j < Lb - 1 || i == n - 1, shared && i == 0 && j == 0);
            }
            skips.push_back({x, hh, ww, ci});
        }
        if (i != n - 1) {
            const int ho = (hh - 1) / 2 + 1, wo = (ww - 1) / 2 + 1;
            Run::G g;
            g.conv = 1; g.B = B; g.Hi = hh; g.Wi = ww; g.Ho = ho; g.Wo = wo; g.stride = 2;
            g.defer = 1;   // -> the next block's norm1
            void* o = R.buf("ds" + std::to_string(i));
            R.gemm(x, 0, B * ho * wo, R.pw("down_blocks." + std::to_string(i) + ".downsamplers.0.conv"), o, g);
            x = o;
            hh = ho; ww = wo;
            skips.push_back({x, hh, ww, ci});
        }
    }
    // ---- 4. mid (ref :775-783)
    const int cm = c.block_out_channels[n - 1];
    x = resnet("mid_block.resnets.0.", x, cm, nullptr, 0, hh * ww, hh, ww, "r", true);
    x = transformer("mid_block.attentions.0.", x, cm, c.heads[n - 1], hh * ww, "r2");
    x = resnet("mid_block.resnets.1.", x, cm, nullptr, 0, hh * ww, hh, ww, "r", !u->freeu);   // (FreeU reads the bf16 tensor: no deferred reduce)
    // ---- 5. up (ref :789-814)
    int cx = cm;
    for (int i = 0; i < n && !R.rc; ++i) {
        const int co = c.block_out_channels[n - 1 - i];
        const bool fu = u->freeu && i < 2;   // FreeU: the backbone scaled in place (nothing else reads it), the filtered skip in "fu_s"
        for (int j = 0; j < Lb + 1; ++j) {
            Skip sk = skips.back();
            skips.pop_back();
            if (sk.hh != hh || sk.ww != ww) { u->err = "skip size mismatch"; return -1; }
            if (fu && !R.rc) {
                void* fs = R.buf("fu_s");
                R.chk(pcdm_freeu(x, const_cast<void*>(x), sk.p, fs, B, hh, ww, cx, sk.ch, u->fu_b[i], u->fu_s[i],
                                 u->bufs.count("fu_ws") ? R.buf("fu_ws") : nullptr, s), "pcdm_freeu");
                sk.p = fs;
            }
            // (a resnet whose output the next resnet's FreeU reads materialises it: no reduce deferred to a GroupNorm)
            x = resnet("up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j) + ".", x, cx, sk.p, sk.ch, hh * ww, hh, ww, (j + i) % 2 ? "r" : "rb",
                       has_cross(c, n - 1 - i) || (j < Lb ? !fu : i == n - 1));
            cx = co;
            if (has_cross(c, n - 1 - i))
                x = transformer("up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j) + ".", x, co, c.heads[n - 1 - i], hh * ww, j % 2 ? "u" : "ub");
        }
        if (i != n - 1) {
            const int ho = skips.back().hh, wo = skips.back().ww;   // = (2 hh, 2 ww) unless a down conv rounded an odd size up
            const std::string up4 = "up_blocks." + std::to_string(i) + ".upsamplers.0.conv4";
            if (u->w.count(up4) && ho == 2 * hh && wo == 2 * ww) {
                // the phase decomposition of conv3x3(nearest x2 (x)) (registered as "...upsamplers.0.conv4": pcdms_amd/ops.py pack_upsample_phases):
                // one 3x3 launch on the low-res tensor with N = 4 C, every output-channel group (= output phase) over its four taps, then the shuffle
                Run::G g4;
                g4.conv = 1; g4.B = B; g4.Hi = hh; g4.Wi = ww; g4.Ho = hh; g4.Wo = ww;
                g4.tap_lut = 0x8754764354214310ull; g4.tap_group_n = cx;
                R.gemm(x, 0, B * hh * ww, R.pw(up4), R.buf("c1"), g4);
                R.chk(pcdm_pixel_shuffle2(R.buf("c1"), R.buf("us"), B, hh, ww, cx, s), "pcdm_pixel_shuffle2");
                x = R.buf("us");
                hh = ho; ww = wo;
                continue;
            }
            Run::G g;
            g.conv = 1; g.B = B; g.Hi = hh; g.Wi = ww; g.Ho = ho; g.Wo = wo; g.upsample = 1;
            g.defer = (u->freeu && i + 1 < 2) ? 0 : 1;   // -> the next block's norm1 (or its FreeU, which reads the bf16 tensor)
            R.gemm(x, 0, B * ho * wo, R.pw("up_blocks." + std::to_string(i) + ".upsamplers.0.conv"), R.buf("us"), g);
            x = R.buf("us");
            hh = ho; ww = wo;
        }
    }
    // ---- 6. post-process (ref :817-820)
    R.groupnorm(x, C0, nullptr, 0, B, HW, eps, R.vec("conv_norm_out.weight"), R.vec("conv_norm_out.bias"), 1, R.buf("gn"));
    {
        Run::G g;
        g.conv = 1; g.B = B; g.Hi = h; g.Wi = w; g.Ho = h; g.Wo = w; g.rows_per_batch = HW; g.epilogue = PCDM_EPI_NCHW_F32;
        R.gemm(R.buf("gn"), 0, B * HW, R.pw("conv_out"), eps_out, g);
    }
    return R.rc;
}

extern "C" int pcdm_unet_forward(pcdm_unet* u, const void* x_in, const int64_t* t_dev, const int32_t* step_dev, int B, int h, int w, int L,
                                 int pose_b, void* workspace, float* eps_out, pcdm_stream_t s) {
    return unet_forward_impl(u, x_in, t_dev, false, step_dev, B, h, w, L, pose_b, workspace, eps_out, s);
}
extern "C" int pcdm_unet_forward_f32(pcdm_unet* u, const void* x_in, const float* t_dev, const int32_t* step_dev, int B, int h, int w, int L,
                                     int pose_b, void* workspace, float* eps_out, pcdm_stream_t s) {
    return unet_forward_impl(u, x_in, t_dev, true, step_dev, B, h, w, L, pose_b, workspace, eps_out, s);
}

// ---- weight packing for hosts without pcdms_amd.ops.pack_* (plain host loops; the caller uploads the result) ---------------------------
namespace {
inline uint16_t host_f2bf(float f) {   // round-to-nearest-even, NaN preserved (the conversion torch's .to(bfloat16) performs)
    uint32_t x;
    memcpy(&x, &f, 4);
    if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((x >> 16) | 0x40);
    x += 0x7fffu + ((x >> 16) & 1u);
    return (uint16_t)(x >> 16);
}
}  // namespace

// nn.Linear / 1x1-conv weight fp32 [N, K] -> bf16 [Npad, K] (rows >= N zero), Npad = N rounded up to pad_to (64); bias -> fp32 [Npad].
// Returns Npad; out_w / out_bias may be NULL to query the size.
extern "C" int pcdm_pack_linear(const float* w, const float* bias, int N, int K, int pad_to, uint16_t* out_w, float* out_bias) {
    if (N <= 0 || K <= 0 || K % 64 || pad_to <= 0) return -1;
    const int Npad = (N + pad_to - 1) / pad_to * pad_to;
    if (out_w) {
        if (!w) return -1;
        for (int64_t n = 0; n < Npad; ++n)
            for (int64_t k = 0; k < K; ++k) out_w[n * K + k] = n < N ? host_f2bf(w[n * K + k]) : 0;
    }
    if (out_bias)
        for (int n = 0; n < Npad; ++n) out_bias[n] = (bias && n < N) ? bias[n] : 0.f;
    return Npad;
}

// Conv2d weight fp32 [N, Cin, 3, 3] -> bf16 [Npad, 9 * Cp], k = (ky * 3 + kx) * Cp + c, Cp = Cin rounded up to 64.  Returns Npad; *K_out = 9 Cp,
// *cin_out = Cp.
extern "C" int pcdm_pack_conv3x3(const float* w, const float* bias, int N, int Cin, int pad_to, uint16_t* out_w, float* out_bias, int* K_out,
                                 int* cin_out) {
    if (N <= 0 || Cin <= 0 || pad_to <= 0) return -1;
    const int Cp = (Cin + 63) / 64 * 64, K = 9 * Cp;
    const int Npad = (N + pad_to - 1) / pad_to * pad_to;
    if (K_out) *K_out = K;
    if (cin_out) *cin_out = Cp;
    if (out_w) {
        if (!w) return -1;
        memset(out_w, 0, (size_t)Npad * K * sizeof(uint16_t));
        for (int64_t n = 0; n < N; ++n)
            for (int c = 0; c < Cin; ++c)
                for (int t = 0; t < 9; ++t) out_w[n * K + t * Cp + c] = host_f2bf(w[(n * Cin + c) * 9 + t]);
    }
    if (out_bias)
        for (int n = 0; n < Npad; ++n) out_bias[n] = (bias && n < N) ? bias[n] : 0.f;
    return Npad;
}

// GEGLU projection fp32 [2 D, K] (rows [h | gate]) + bias [2 D] -> bf16 [2 Dp, K] with rows interleaved per 64 as [32 h | 32 gate]
// (Dp = D rounded up to 64), bias likewise.  Returns Npad = 2 Dp; the GEMM's N is D.
extern "C" int pcdm_pack_geglu(const float* w, const float* bias, int D, int K, uint16_t* out_w, float* out_bias) {
    if (D <= 0 || K <= 0 || K % 64) return -1;
    const int Dp = (D + 63) / 64 * 64;
    for (int64_t r = 0; r < 2 * Dp && (out_w || out_bias); ++r) {
        const int blk = (int)(r / 64), in = (int)(r % 64);
        const int d = blk * 32 + (in & 31);          // output channel
        const bool gate = in >= 32;
        const int64_t src = gate ? (int64_t)D + d : d;
        if (out_w) {
            if (!w) return -1;
            for (int64_t k = 0; k < K; ++k) out_w[r * K + k] = d < D ? host_f2bf(w[src * K + k]) : 0;
        }
        if (out_bias) out_bias[r] = (bias && d < D) ? bias[src] : 0.f;
    }
    return 2 * Dp;
}
