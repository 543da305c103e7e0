// U-Net-to-tap graph executor and its C ABI (dsim_unet_*; the ops' and score tails' entry points are in api.hip).
//
// Implements, as a sequence of hand-written gfx950 kernels on ONE HIP stream, the sub-graph of
// diffusers' UNet2DConditionModel that the reference executes before its attention pre-hook
// fires (DiffSimPipeline.step -> self.unet(...), /root/reference/diffsim/diffsim_pipeline.py:213;
// hook at /root/reference/diffsim/diffsim.py:43-56).  Block control flow follows the reference's
// own restatement of it:
//   CrossAttnDownBlock2D  hacked_modules.py:537-620     UNetMidBlock2DCrossAttn  :622-688
//   CrossAttnUpBlock2D    hacked_modules.py:438-535     Transformer2DModel       :261-434
//   BasicTransformerBlock hacked_modules.py:17-136      q/k/v tap                hacked_attn.py:61-77
// and stops at the tap (nothing downstream of it feeds q/k/v).
//
// One `walk()` serves three purposes: PLAN (dry run: peak workspace bytes), RUN (launch), so the
// planner can never disagree with the executor.  Activations are token-major [B][HW][C] in the
// compute dtype; the workspace is a caller-provided arena with stack discipline.
#include <array>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "store.h"

using namespace dsim;

struct dsim_unet : WeightStore {
    dsim_unet_cfg cfg;
    int timestep = -1;
    float* temb = nullptr;          // [time_embed_dim]
    float* tscratch = nullptr;      // time-embedding scratch
    bool two_temb = false;          // SDXL: the CFG halves carry different time embeddings
    bool cfg_dedup = false;         // opt-in: compute the part of the graph that is identical in both CFG halves once
    int fusion = DSIM_FUSE_ALL;     // dsim_unet_set_fusion mask: which multi-op kernels replace their unfused chains
};

namespace {

// One tap of a walk: the dsim_unet_cfg fields of the same names (tap_attn / tap_tfm -1 = the last one) and the tensors that receive
// its q, k, v.  A walk captures every tap it passes and ends at the deepest.
struct TapReq {
    int block, layer, attn, tfm;
    void *q = nullptr, *k = nullptr, *v = nullptr;
};

// the handle's own tap as a one-tap request
static std::vector<TapReq> cfg_taps(const dsim_unet_cfg& c) { return {TapReq{c.tap_block, c.tap_layer, c.tap_attn, c.tap_tfm}}; }

// ---- the walk ----------------------------------------------------------------------------
// The rows a step of a transformer block works on: the residual stream, the attention output (which then holds the cross-attention
// query) and their batch elements.
struct Rows {
    void* h = nullptr;
    void* a = nullptr;
    int B = 0;
};
// One Transformer2DModel under way: its geometry and the buffers its blocks share.  `full` is the whole batch; `half` exists under
// CFG de-duplication only (one row set per image: the first block runs on it up to its cross-attention query, then the halves part).
struct Tfm {
    int C = 0, HW = 0, heads = 0;
    Rows full, half;
    const void* x = nullptr;    // the model's input, the residual of proj_out (de-duplicated: one copy per image ...
    void* xfull = nullptr;      //   ... and its [image][cfg] copy, written where the halves part)
    void* nb = nullptr;         // LayerNorm outputs
    void* big = nullptr;        // qkv [M][3C], the cross-attention output, the GEGLU output [M][4C]
    void* kvb = nullptr;        // the prompt context's K | V
};

struct Walk : WalkBase<dsim_unet> {
    const int B2;           // U-Net batch of the call = 2 * images (CFG); a step's own batch is its input's (Act.B)
    void* gn_scratch = nullptr;
    void* ctx_t = nullptr;  // [2][L][Dc] compute dtype; with a context table, [B2][L][Dc] (one context per batch element)
    std::vector<TapReq> taps;   // where q, k, v are captured; the walk ends at the deepest of them
    int n_captured = 0;
    bool tapped = false;        // every tap captured
    int n_ctx = 1;              // prompt contexts of the call: > 1 = a table of [uncond, cond] pairs, one row per image
    const int32_t* ctx_index = nullptr;     // device int32 [images]: each image's row of the table (n_ctx > 1)
    bool mixed() const { return n_ctx > 1; }
    // the text request (dsim_unet_qkv_text, an own-tap walk): the walk does not stop at the tap but runs the block on to its
    // cross-attention's query and K | V projection, written here
    void* text_xq = nullptr;    // [B2][HW][C]
    void* text_xkv = nullptr;   // [2 or B2][L][2C]
    bool text = false;

    Walk(dsim_unet* h, Arena* ar, hipStream_t s, int B2, bool run) : WalkBase(h, ar, s, run), B2(B2) {}

    int linear(const void* a0, int c0, const void* a1, int c1, const Packed* w, const Packed* b, const void* residual,
               void* out, int M, int N, int ldo, int epi = -1) {
        GemmArgs g = linear_args(a0, c0, w->p, b ? (const float*)b->p : nullptr, residual, out, M, N);
        if (a1) { g.A1 = a1; g.C1 = c1; g.K = c0 + c1; }
        g.ldo = ldo;
        if (epi >= 0) g.epi = epi;
        if (g.epi == EPI_GEGLU) g.geglu_blk = geglu_block_rows(N);       // as pack_all() interleaved it
        return gemm(g);
    }
    int conv3(const Act& x, const Packed* w, const float* bias, const void* residual, void* out, int Cout, int stride,
              int ups, const float* bias_odd = nullptr) {
        GemmArgs g = conv3_args(x, w->p, bias, residual, out, Cout, stride, ups, 1);
        if (h->two_temb && bias_odd) { g.bias2 = bias_odd; g.rows_per_batch = g.Hout * g.Wout; }
        return gemm(g);
    }
    int gn(const Act& x0, const Act* x1, const Packed* g, const Packed* b, void* out, float eps, int silu) {
        const int HW = x0.H * x0.W, C1 = x1 ? x1->C : 0, groups = h->cfg.norm_num_groups;
        if (run && !out) return DSIM_ERR_INVALID;
        return launch([&] { return gn_rec(x0.B, HW, x0.C, C1, groups); },
                      [&] {
                          return launch_groupnorm(x0.p, x0.C, x1 ? x1->p : nullptr, C1, (const float*)g->p, (const float*)b->p, out, x0.B, HW,
                                                  groups, eps, silu, h->dt, gn_scratch, s);
                      });
    }
    int ln(const void* x, const Packed* g, const Packed* b, void* out, int M, int C) {
        if (run && !out) return DSIM_ERR_INVALID;
        return launch([&] { return rec(std::string("layernorm_") + dtn() + "|M" + std::to_string(M) + " C" + std::to_string(C), 0.0,
                                       2.0 * M * (double)C * es()); },
                      [&] { return launch_layernorm(x, (const float*)g->p, (const float*)b->p, out, M, C, 1e-5f, h->dt, s); });
    }
    int attn(const AttnArgs& a) {
        return launch([&] { return attn_rec(a); }, [&] { return launch_attention(a, h->dt, s); });
    }
    // Does the level of HW-row maps take the row-resident forms that came after the 320-channel LayerNorm ones (the 640-channel
    // LayerNorm forms, the GroupNorm form)?  Whole 128-row tiles per image: the map size decides, never the batch.
    static bool rowres_level(int HW) { return HW % 128 == 0; }
    // Which normalisations run inside their consumer's row-resident launch: each decided here once, for the launches below and for
    // transformer(), which allocates the normalised-rows buffer only where one of them does not.
    const Packed* ln_proj_stream(const std::string& key, int C, int HW) const {        // LayerNorm + projection (C = 320; C = 640 on a rowres_level)
        const auto it = h->pk.find(key);
        return (it == h->pk.end() || !(h->fusion & DSIM_FUSE_LNPROJ) || (C != 320 && !rowres_level(HW))) ? nullptr : &it->second;
    }
    const Packed* gn_proj_stream(const std::string& p, int HW) const {                 // GroupNorm + proj_in (a rowres_level)
        const auto it = h->pk.find(p + "proj_in.stream");
        return (it == h->pk.end() || !(h->fusion & DSIM_FUSE_LNPROJ) || !rowres_level(HW)) ? nullptr : &it->second;
    }
    const Packed* ff_stream(const std::string& b) const {                              // the whole feed-forward behind norm3
        const auto it = h->pk.find(b + "ff.stream");
        return (it == h->pk.end() || !(h->fusion & DSIM_FUSE_FF)) ? nullptr : &it->second;
    }
    // LayerNorm + projection as one row-resident launch where the width has one (16-bit modes).  Returns 1 where it has none: the
    // caller runs the unfused chain.
    int ln_proj(const void* x, const Packed* g, const Packed* b, const std::string& key, void* out, int M, int C, int N, int HW) {
        const Packed* st = ln_proj_stream(key, C, HW);
        if (!st) return 1;
        return launch([&] { return rec(std::string("ln_linear_") + dtn() + "|M" + std::to_string(M) + " N" + std::to_string(N) + " K" +
                                           std::to_string(C), 2.0 * M * (double)C * N, (double)M * (C + N) * es() + (double)C * N * es()); },
                      [&] {
                          RowLinArgs ra;
                          ra.x = x; ra.out = out; ra.ln_g = (const float*)g->p; ra.ln_b = (const float*)b->p; ra.stream = st->p;
                          ra.M = M; ra.C = C; ra.N = N; ra.eps = 1e-5f; ra.dtype = h->dt;
                          return launch_rowlin(ra, s);
                      });
    }
    // GroupNorm + proj_in of a Transformer2DModel as a statistics pass and one row-resident launch that normalises the rows on arrival
    // (16-bit modes, C = 320 / 640).  coef: the statistics pass's table, [x.B][2][C] f32.  Returns 1 where there is none: the caller
    // runs gn() and linear().
    int gn_proj(const std::string& p, const Act& x, const Packed* g, const Packed* b, const Packed* bias, float* coef, void* out) {
        const int HW = x.H * x.W, C = x.C, M = x.rows(), groups = h->cfg.norm_num_groups;
        const Packed* st = gn_proj_stream(p, HW);
        if (!st) return 1;
        const std::string shape = "|B" + std::to_string(x.B) + " HW" + std::to_string(HW) + " C" + std::to_string(C);
        CK(launch([&] { return rec(std::string("groupnorm_stats_") + dtn() + shape, 0.0, (double)M * C * es()); },
                  [&] {
                      return launch_groupnorm_stats(x.p, C, (const float*)g->p, (const float*)b->p, x.B, HW, groups, 1e-6f, h->dt, gn_scratch,
                                                    coef, s);
                  }));
        return launch([&] { return rec(std::string("gn_linear_") + dtn() + "|M" + std::to_string(M) + " N" + std::to_string(C) + " K" +
                                           std::to_string(C), 2.0 * M * (double)C * C, 2.0 * M * (double)C * es() + (double)C * C * es()); },
                      [&] {
                          RowLinArgs ra;
                          ra.x = x.p; ra.out = out; ra.stream = st->p; ra.M = M; ra.C = C; ra.N = C; ra.dtype = h->dt;
                          ra.gn = 1; ra.coef = coef; ra.bias = (const float*)bias->p; ra.HW = HW;
                          return launch_rowlin(ra, s);
                      });
    }

    // ResnetBlock2D; x1 = skip tensor concatenated after x0 on channels
    int resnet(const std::string& p, const Act& x0, const Act* x1, int Cout, Act* out) {
        const int Cin = x0.C + (x1 ? x1->C : 0), B = x0.B, H = x0.H, W = x0.W, M = x0.rows();
        WGET(n1w, p + "norm1.weight"); WGET(n1b, p + "norm1.bias");
        WGET(c1w, p + "conv1.weight"); WGET(c1b, p + "conv1.bias_eff"); WGET(c1b2, p + "conv1.bias_eff2");
        WGET(n2w, p + "norm2.weight"); WGET(n2b, p + "norm2.bias");
        WGET(c2w, p + "conv2.weight"); WGET(c2b, p + "conv2.bias");
        *out = act(B, H, W, Cout);
        const size_t mk = ar->mark();
        const Act t1 = act(B, H, W, Cin);
        CK(gn(x0, x1, n1w, n1b, t1.p, h->cfg.norm_eps, 1));
        const Act t2 = act(B, H, W, Cout);
        CK(conv3(t1, c1w, (const float*)c1b->p, nullptr, t2.p, Cout, 1, 0, (const float*)c1b2->p));
        const Act t3 = act(B, H, W, Cout);
        CK(gn(t2, nullptr, n2w, n2b, t3.p, h->cfg.norm_eps, 1));
        const void* res = x0.p;
        if (Cin != Cout) {
            WGET(scw, p + "conv_shortcut.weight"); WGET(scb, p + "conv_shortcut.bias");
            void* sc = alloc_act((size_t)M * Cout);
            CK(linear(x0.p, x0.C, x1 ? x1->p : nullptr, x1 ? x1->C : 0, scw, scb, nullptr, sc, M, Cout, Cout));
            res = sc;
        } else if (x1) {
            return DSIM_ERR_INVALID;
        }
        CK(conv3(t3, c2w, (const float*)c2b->p, res, out->p, Cout, 1, 0));
        ar->release(mk);
        return DSIM_OK;
    }

    int heads_at(int level) const { return h->cfg.heads_per_level[level] > 0 ? h->cfg.heads_per_level[level] : h->cfg.num_heads; }
    int depth_at(int level) const { return h->cfg.depth_per_level[level] > 0 ? h->cfg.depth_per_level[level] : 1; }

    // the requested taps in the Transformer2DModel of (block, layer, attention j) -- indices into `taps`; nattn: attentions of the block
    std::vector<int> site(int block, int layer, int j, int nattn) const {
        std::vector<int> r;
        for (int t = 0; t < (int)taps.size(); ++t) {
            const TapReq& q = taps[t];
            if (q.block != block) continue;
            if (block == DSIM_TAP_MID || (q.layer == layer && j == (q.attn < 0 ? nattn - 1 : q.attn))) r.push_back(t);
        }
        return r;
    }

    // hacked_attn.py:61-69: to_q / to_k / to_v of the normed block input nb, no bias; written [B][N][H*D] to the tap's tensors
    int tap_qkv(const void* nb, const Packed* qkv, int C, int M, const TapReq& t) {
        Packed wq = *qkv, wk = *qkv, wv = *qkv;
        wk.p = (char*)qkv->p + (size_t)C * C * es();
        wv.p = (char*)qkv->p + (size_t)2 * C * C * es();
        // one launch when q, k, v lie at equal distances (engine.py allocates them as one [3][...] buffer) and the width
        // tiles by 320: the packed [3C][C] weight as one N = 3C GEMM whose column runs go to the three tensors
        const long long qk = (const char*)t.k - (const char*)t.q, kv = (const char*)t.v - (const char*)t.k;
        const bool bm_split = C % 320 == 0;
        if ((h->fusion & DSIM_FUSE_TAPQKV) && qk == kv && qk >= (long long)M * C * (long long)es() && 3 * qk < 0x7fffffffll && bm_split) {
            GemmArgs g = linear_args(nb, C, qkv->p, nullptr, nullptr, t.q, M, 3 * C);
            g.ldo = C; g.out_split = C; g.out_split_stride = qk;
            return gemm(g);
        }
        CK(linear(nb, C, nullptr, 0, &wq, nullptr, nullptr, t.q, M, C, C));
        CK(linear(nb, C, nullptr, 0, &wk, nullptr, nullptr, t.k, M, C, C));
        return linear(nb, C, nullptr, 0, &wv, nullptr, nullptr, t.v, M, C, C);
    }

    // ---- BasicTransformerBlock `b` of the model t, in its three parts (hacked_modules.py:17-136) ------------------------------------
    // Self-attention on the rows r.  here: the taps of this block (indices into `taps`).  At a tapped block, norm1 and the q/k/v
    // projection run as a walk that stops there runs them; `last`: the walk holds every tap after this block's -- it ends here
    // (tapped = true), and the caller unwinds.
    int self_attention(const std::string& b, const Tfm& t, const Rows& r, const std::vector<int>& here, bool last) {
        const int C = t.C, M = r.B * t.HW;
        WGET(l1w, b + "norm1.weight"); WGET(l1b, b + "norm1.bias");
        WGET(qkv, b + "attn1.qkv");
        // (the fused launch: not in the block the walk ends in, whose q, k, v go to three tensors)
        const int fq = last ? 1 : ln_proj(r.h, l1w, l1b, b + "attn1.qkv.stream", t.big, M, C, 3 * C, t.HW);
        if (fq < 0) return fq;
        // a tap's q/k/v come from the unfused norm1 -> projection chain: the fused launch is not bit-identical to it, so where the
        // block carries on through that launch, the tap gets a norm1 of its own; elsewhere the two share one
        if (fq > 0 || !here.empty()) CK(ln(r.h, l1w, l1b, t.nb, M, C));
        for (int i : here) {
            CK(tap_qkv(t.nb, qkv, C, M, taps[i]));
            ++n_captured;
        }
        if (last && !text) {
            tapped = true;
            return DSIM_OK;
        }
        WGET(o1w, b + "attn1.to_out.0.weight"); WGET(o1b, b + "attn1.to_out.0.bias");
        if (last) {
            // the text walk: the self-attention on the tap's own tensors (no second projection), to_out + residual, then the
            // cross-attention's query and the prompt's K | V into the caller's tensors; the walk ends behind them
            const TapReq& tp = taps[here.back()];
            AttnArgs a;
            a.q = tp.q; a.ldq = C; a.k = tp.k; a.v = tp.v; a.ldk = C;
            a.out = r.a; a.ldo = C; a.B = r.B; a.Bkv = r.B; a.H = t.heads; a.Nq = t.HW; a.Nk = t.HW; a.D = C / t.heads;
            CK(attn(a));
            CK(linear(r.a, C, nullptr, 0, o1w, o1b, r.h, r.h, M, C, C));
            CK(cross_query(b, t, r, text_xq));
            CK(cross_kv(b, t, text_xkv));
            tapped = true;
            return DSIM_OK;
        }
        if (fq > 0) CK(linear(t.nb, C, nullptr, 0, qkv, nullptr, nullptr, t.big, M, 3 * C, 3 * C));
        AttnArgs a;
        a.q = t.big; a.ldq = 3 * C;
        a.k = (char*)t.big + (size_t)C * es(); a.v = (char*)t.big + (size_t)2 * C * es(); a.ldk = 3 * C;
        a.out = r.a; a.ldo = C; a.B = r.B; a.Bkv = r.B; a.H = t.heads; a.Nq = t.HW; a.Nk = t.HW; a.D = C / t.heads;
        CK(attn(a));
        return linear(r.a, C, nullptr, 0, o1w, o1b, r.h, r.h, M, C, C);
    }

    // The two CFG halves part: [image] -> [image][cfg] for the residual stream, the cross-attention query and the model's input.
    int part_halves(const Tfm& t) {
        const int n = t.half.B;
        const size_t per = (size_t)t.HW * t.C * es();
        return launch([&] { return rec(std::string("cfg_duplicate_") + dtn(), 0.0, 3.0 * 3.0 * (n * t.HW) * (double)t.C * es()); },
                      [&] {
                          int st = dup_batch(t.half.h, t.full.h, n, per, s);
                          if (st == DSIM_OK) st = dup_batch(t.half.a, t.full.a, n, per, s);
                          if (st == DSIM_OK) st = dup_batch(t.x, t.xfull, n, per, s);
                          return st;
                      });
    }

    // The query part of a cross-attention, the last thing computed on the rows r: norm2 -> attn2.to_q, as one row-resident launch
    // where the fusion mask and the width have one, into xq ([r.B][HW][C]; cross_attention passes r.a, the text walk the caller's).
    int cross_query(const std::string& b, const Tfm& t, const Rows& r, void* xq) {
        const int C = t.C;
        WGET(l2w, b + "norm2.weight"); WGET(l2b, b + "norm2.bias");
        WGET(q2w, b + "attn2.to_q.weight");
        const int f2 = ln_proj(r.h, l2w, l2b, b + "attn2.to_q.stream", xq, r.B * t.HW, C, C, t.HW);
        if (f2 < 0) return f2;
        if (f2 > 0) {
            CK(ln(r.h, l2w, l2b, t.nb, r.B * t.HW, C));
            CK(linear(t.nb, C, nullptr, 0, q2w, nullptr, nullptr, xq, r.B * t.HW, C, C));
        }
        return DSIM_OK;
    }
    // The prompt's K | V of a cross-attention into kvb, [2][L][2C] -- with a context table every batch element projects its own
    // context, [B][L][2C], and attends to its own K / V
    int cross_kv(const std::string& b, const Tfm& t, void* kvb) {
        const int C = t.C, L = h->cfg.ctx_len, Dc = h->cfg.cross_attention_dim;
        WGET(kv2, b + "attn2.kv");
        const int Bkv = mixed() ? t.full.B : 2;
        return linear(ctx_t, Dc, nullptr, 0, kv2, nullptr, nullptr, kvb, Bkv * L, 2 * C, 2 * C);
    }

    // Cross-attention against the prompt context: batch element b uses ctx[b % 2]; with a context table (n_ctx > 1),
    // ctx[index[b / 2]][b % 2], gathered per batch element in go().  The query is the last thing computed on the rows r; the prompt
    // enters after it, so `pre` (r = the de-duplicated half) parts the halves there and the rest runs on the full batch.
    int cross_attention(const std::string& b, const Tfm& t, const Rows& r, bool pre) {
        const int C = t.C, L = h->cfg.ctx_len;
        WGET(o2w, b + "attn2.to_out.0.weight"); WGET(o2b, b + "attn2.to_out.0.bias");
        CK(cross_query(b, t, r, r.a));
        if (pre) CK(part_halves(t));
        const Rows& f = t.full;
        const int Bkv = mixed() ? f.B : 2;
        CK(cross_kv(b, t, t.kvb));
        AttnArgs a;
        a.q = f.a; a.ldq = C;
        a.k = t.kvb; a.v = (char*)t.kvb + (size_t)C * es(); a.ldk = 2 * C;
        a.out = t.big; a.ldo = C; a.B = f.B; a.Bkv = Bkv; a.H = t.heads; a.Nq = t.HW; a.Nk = L; a.D = C / t.heads;
        CK(attn(a));
        return linear(t.big, C, nullptr, 0, o2w, o2b, f.h, f.h, f.B * t.HW, C, C);
    }

    // Feed-forward: norm3 -> Linear(C,8C) -> h*gelu(g) -> Linear(4C,C) -> + residual.  One row-resident launch where the width has
    // one (16-bit modes, C = 320); else LayerNorm, the GEGLU GEMM (h*gelu(g) in its epilogue) and ff.net.2.
    int feed_forward(const std::string& b, const Tfm& t) {
        const int C = t.C, M = t.full.B * t.HW;
        void* hb = t.full.h;
        WGET(l3w, b + "norm3.weight"); WGET(l3b, b + "norm3.bias");
        WGET(f1w, b + "ff.net.0.proj.weight"); WGET(f1b, b + "ff.net.0.proj.bias");
        WGET(f2w, b + "ff.net.2.weight"); WGET(f2b, b + "ff.net.2.bias");
        if (const Packed* fst = ff_stream(b))
            return launch([&] { return rec(std::string("ff_fused_") + dtn() + "|M" + std::to_string(M) + " C" + std::to_string(C),
                                           2.0 * M * (double)C * 12 * C, 2.0 * M * (double)C * es() + 12.0 * C * C * es()); },
                          [&] {
                              FFArgs fa;
                              fa.x = hb; fa.out = hb; fa.ln_g = (const float*)l3w->p; fa.ln_b = (const float*)l3b->p;
                              fa.stream = fst->p; fa.b1 = (const float*)f1b->p; fa.b2 = (const float*)f2b->p; fa.M = M; fa.C = C;
                              fa.eps = 1e-5f; fa.dtype = h->dt;
                              return launch_ff_fused(fa, s);
                          });
        CK(ln(hb, l3w, l3b, t.nb, M, C));
        CK(linear(t.nb, C, nullptr, 0, f1w, f1b, nullptr, t.big, M, 8 * C, 4 * C, EPI_GEGLU));
        return linear(t.big, 4 * C, nullptr, 0, f2w, f2b, hb, hb, M, C, C);
    }

    // Transformer2DModel (GroupNorm -> proj_in -> `depth` BasicTransformerBlocks -> proj_out -> +residual; the
    // conv1x1 and the Linear form of proj_in/out are the same GEMM on token-major data).  caps: the requested taps here (site()).
    // The walk stops in the block that holds its last tap, or every block carries on exactly as an untapped one.
    // half_in: x holds ONE copy per image (opt-in CFG de-duplication): everything up to the first cross-attention -- the first
    // place the prompt context enters -- runs on that half batch, then the residual stream, the model's input and the
    // cross-attention query are duplicated into [image][cfg] order (part_halves) and the rest runs as usual.
    int transformer(const std::string& p, const Act& x, int level, const std::vector<int>& caps, Act* out, bool half_in = false) {
        const int C = x.C, HW = x.H * x.W, B = half_in ? 2 * x.B : x.B, M = B * HW, depth = depth_at(level);
        std::vector<int> cap_blk(caps.size());           // transformer block of each tap here
        int last_blk = -1;
        for (size_t i = 0; i < caps.size(); ++i) {
            const int tb = taps[caps[i]].tfm < 0 ? depth - 1 : taps[caps[i]].tfm;
            if (tb >= depth) return DSIM_ERR_INVALID;
            cap_blk[i] = tb;
            if (tb > last_blk) last_blk = tb;
        }
        // the walk ends in this model when it holds every tap not captured yet: after norm1 and q/k/v of block last_blk
        const bool stop_here = !caps.empty() && n_captured + (int)caps.size() == (int)taps.size();
        if (!stop_here) last_blk = -1;
        WGET(gnw, p + "norm.weight"); WGET(gnb, p + "norm.bias");
        WGET(piw, p + "proj_in.weight"); WGET(pib, p + "proj_in.bias");
        if (!stop_here) *out = act(B, x.H, x.W, C);
        const size_t mk = ar->mark();
        Tfm t;
        t.C = C; t.HW = HW; t.heads = heads_at(level); t.x = x.p;
        // nb: the GroupNorm's output, dead after proj_in, then the LayerNorm outputs.  A model whose every normalisation runs inside
        // its consumer's launch (no tap here: a tap has a norm1 of its own) has none; gn() and ln() refuse a null output.
        const bool gnp = gn_proj_stream(p, HW) != nullptr;
        bool all_fused = gnp && caps.empty();
        for (int blk = 0; blk < depth && all_fused; ++blk) {
            const std::string b = p + "transformer_blocks." + std::to_string(blk) + ".";
            all_fused = ln_proj_stream(b + "attn1.qkv.stream", C, HW) && ln_proj_stream(b + "attn2.to_q.stream", C, HW) && ff_stream(b);
        }
        if (!all_fused) t.nb = alloc_act((size_t)M * C);
        float* const coef = gnp ? (float*)ar->alloc((size_t)x.B * 2 * C * sizeof(float)) : nullptr;      // the statistics pass's table
        t.full.h = alloc_act((size_t)M * C); t.full.B = B;
        if (half_in) {
            t.half.h = alloc_act((size_t)x.rows() * C); t.half.a = alloc_act((size_t)x.rows() * C); t.half.B = x.B;
            t.xfull = alloc_act((size_t)M * C);
            for (int tb : cap_blk)
                if (tb == 0) return DSIM_ERR_INVALID;    // (callers never de-duplicate a tapped first block)
        }
        const int fp = gn_proj(p, x, gnw, gnb, pib, coef, half_in ? t.half.h : t.full.h);
        if (fp < 0) return fp;
        if (fp > 0) {
            CK(gn(x, nullptr, gnw, gnb, t.nb, 1e-6f, 0));
            CK(linear(t.nb, C, nullptr, 0, piw, pib, nullptr, half_in ? t.half.h : t.full.h, x.rows(), C, C));
        }
        for (int blk = 0; blk < depth; ++blk) {
            const std::string b = p + "transformer_blocks." + std::to_string(blk) + ".";
            const bool pre = half_in && blk == 0, last = blk == last_blk;
            if (!last && !t.big) {
                // qkv [M][3C]; later the GEGLU output [M][4C] unless the feed-forward runs as one launch
                const bool ff1 = ff_stream(b) != nullptr;
                t.big = alloc_act((size_t)M * (ff1 ? 3 : 4) * C);
                t.full.a = alloc_act((size_t)M * C);
                t.kvb = alloc_act((size_t)(mixed() ? B : 2) * h->cfg.ctx_len * 2 * C);
            } else if (last && text && !t.full.a) {
                t.full.a = alloc_act((size_t)M * C);     // the text walk's attention output (its query and K | V are the caller's)
            }
            std::vector<int> here;
            for (size_t i = 0; i < caps.size(); ++i)
                if (cap_blk[i] == blk) here.push_back(caps[i]);
            const Rows& r = pre ? t.half : t.full;
            CK(self_attention(b, t, r, here, last));
            if (tapped) break;
            CK(cross_attention(b, t, r, pre));
            CK(feed_forward(b, t));
        }
        if (!tapped) {
            WGET(pow_, p + "proj_out.weight"); WGET(pob, p + "proj_out.bias");
            CK(linear(t.full.h, C, nullptr, 0, pow_, pob, half_in ? t.xfull : x.p, out->p, M, C, C));
        }
        ar->release(mk);
        return DSIM_OK;
    }

    int go(const float* lat, const float* noise, float sa, float sb, const float* ctx) {
        const dsim_unet_cfg& c = h->cfg;
        const int nl = c.n_levels, S = c.sample_size, ch0 = c.block_out_channels[0];
        const int L = c.ctx_len, Dc = c.cross_attention_dim;
        gn_scratch = ar->alloc(groupnorm_scratch_bytes(B2, c.norm_num_groups));
        if (mixed()) {
            // one [uncond, cond] context per image, in the [image][cfg] order of the batch: every cross-attention's K / V projection
            // then runs on B2 * L rows (nothing before the first cross-attention depends on the prompt)
            ctx_t = alloc_act((size_t)B2 * L * Dc);
            CK(launch([&] { return rec(std::string("ctx_gather_") + dtn(), 0.0, (double)B2 * L * Dc * (4.0 + es())); },
                      [&] { return gather_ctx(ctx, n_ctx, ctx_index, ctx_t, h->dt, B2 / 2, (size_t)L * Dc, s); }));
        } else {
            ctx_t = ar->alloc((size_t)2 * L * Dc * es());
            CK(launch([&] { return convert_f32_to(ctx, ctx_t, h->dt, (size_t)2 * L * Dc, s); }));
        }
        WGET(ciw, "conv_in.weight"); WGET(cib, "conv_in.bias");
        const auto conv_in = [&](const Act& o, int dup) {
            return prep_conv_in(lat, noise, sa, sb, (const float*)ciw->p, (const float*)cib->p, o.p, h->dt, B2 / 2, c.in_channels, S, ch0, dup, s);
        };
        Act x = act(B2, S, S, ch0);
        CK(launch([&] { return rec("prep_conv_in", 2.0 * B2 * S * S * (double)ch0 * 9 * c.in_channels, (double)B2 * S * S * ch0 * es()); },
                  [&] { return conv_in(x, 2); }));
        std::vector<Act> skips;
        skips.push_back(x);
        // Opt-in CFG de-duplication (dsim_unet_set_cfg_dedup): the reference feeds torch.cat([latents] * 2) with [negative,
        // positive] prompt embeddings (diffsim_pipeline.py:208-221), so conv_in, the first ResnetBlock2D and the first
        // transformer up to its cross-attention query see two bit-identical batch halves.  With one time embedding for both
        // halves (SD1.5; SDXL's text_time embedding differs per half) and the tap outside that block, they are computed once
        // per image -- conv_in a second time, one copy per image, and the first resnet and transformer on that half batch -- and
        // duplicated where the prompt context first enters.  Same kernels, batch-invariant: same bits.
        bool tap_down0 = false;             // a requested tap in the first down block
        for (const TapReq& t : taps) tap_down0 = tap_down0 || (t.block == DSIM_TAP_DOWN && t.layer == 0);
        const bool dedup = h->cfg_dedup && !h->two_temb && c.down_has_attn[0] && c.layers_per_block >= 1 && !tap_down0;
        Act xh;
        if (dedup) {
            xh = act(B2 / 2, S, S, ch0);
            CK(launch([&] { return conv_in(xh, 1); }));
        }
        // ---- down path (hacked_modules.py:583-618) ---------------------------------------
        for (int i = 0; i < nl; ++i) {
            const int co = c.block_out_channels[i];
            const std::string bp = "down_blocks." + std::to_string(i) + ".";
            for (int j = 0; j < c.layers_per_block; ++j) {
                const bool half = dedup && i == 0 && j == 0;
                Act r;
                CK(resnet(bp + "resnets." + std::to_string(j) + ".", half ? xh : x, nullptr, co, &r));
                x = r;
                if (c.down_has_attn[i]) {
                    Act t;
                    CK(transformer(bp + "attentions." + std::to_string(j) + ".", x, i, site(DSIM_TAP_DOWN, i, j, c.layers_per_block), &t,
                                   half));
                    if (tapped) return DSIM_OK;
                    x = t;
                }
                skips.push_back(x);
            }
            if (i != nl - 1) {
                WGET(dw, bp + "downsamplers.0.conv.weight"); WGET(db, bp + "downsamplers.0.conv.bias");
                const Act d = act(x.B, (x.H + 1) / 2, (x.W + 1) / 2, co);
                CK(conv3(x, dw, (const float*)db->p, nullptr, d.p, co, 2, 0));
                x = d;
                skips.push_back(x);
            }
        }
        // ---- mid (hacked_modules.py:632,664-675) -------------------------------------------
        {
            const int cm = c.block_out_channels[nl - 1];
            Act r;
            CK(resnet("mid_block.resnets.0.", x, nullptr, cm, &r));
            x = r;
            Act t;
            CK(transformer("mid_block.attentions.0.", x, nl - 1, site(DSIM_TAP_MID, 0, 0, 1), &t));
            if (tapped) return DSIM_OK;
            x = t;
            CK(resnet("mid_block.resnets.1.", x, nullptr, cm, &r));
            x = r;
        }
        // ---- up path (hacked_modules.py:457-527) -------------------------------------------
        for (int i = 0; i < nl; ++i) {
            const int co = c.block_out_channels[nl - 1 - i];
            const std::string bp = "up_blocks." + std::to_string(i) + ".";
            const int nres = c.layers_per_block + 1;
            for (int j = 0; j < nres; ++j) {
                if (skips.empty()) return DSIM_ERR_INVALID;
                Act sk = skips.back();
                skips.pop_back();
                Act r;
                CK(resnet(bp + "resnets." + std::to_string(j) + ".", x, &sk, co, &r));
                x = r;
                if (c.up_has_attn[i]) {
                    Act t;
                    CK(transformer(bp + "attentions." + std::to_string(j) + ".", x, nl - 1 - i, site(DSIM_TAP_UP, i, j, nres), &t));
                    if (tapped) return DSIM_OK;
                    x = t;
                }
            }
            if (i != nl - 1) {
                WGET(uw, bp + "upsamplers.0.conv.weight"); WGET(ub, bp + "upsamplers.0.conv.bias");
                // the upsampled size is the next skip's (diffusers' upsample_size, hacked_modules.py:531-533): twice the side
                // except below an odd level, where the nearest-neighbour resize to the explicit size runs as its own launch
                const int th = skips.empty() ? x.H * 2 : skips.back().H, tw = skips.empty() ? x.W * 2 : skips.back().W;
                const Act u = act(x.B, th, tw, co);
                if (th == 2 * x.H && tw == 2 * x.W) {
                    CK(conv3(x, uw, (const float*)ub->p, nullptr, u.p, co, 1, 1));      // x2 folded into the conv's gather
                } else {
                    const Act rz = act(x.B, th, tw, co);
                    CK(launch([&] { return rec(std::string("resize_nearest_") + dtn(), 0.0, 2.0 * x.B * th * tw * (double)co * es()); },
                              [&] { return resize_nearest(x.p, rz.p, x.B, x.H, x.W, th, tw, (size_t)co * es(), s); }));
                    CK(conv3(rz, uw, (const float*)ub->p, nullptr, u.p, co, 1, 0));
                }
                x = u;
            }
        }
        return DSIM_ERR_INVALID;   // a tap was never reached: bad tap_block / tap_layer
    }
};

int tap_geometry(const dsim_unet_cfg& c, int* tokens, int* heads, int* hd) {
    const int nl = c.n_levels;
    int level;   // resolution level of the tapped block
    if (c.tap_block == DSIM_TAP_DOWN) {
        if (c.tap_layer < 0 || c.tap_layer >= nl || !c.down_has_attn[c.tap_layer]) return DSIM_ERR_INVALID;
        if (c.tap_attn >= c.layers_per_block) return DSIM_ERR_INVALID;
        level = c.tap_layer;
    } else if (c.tap_block == DSIM_TAP_MID) {
        if (c.tap_attn > 0) return DSIM_ERR_INVALID;
        level = nl - 1;
    } else if (c.tap_block == DSIM_TAP_UP) {
        const int i = c.tap_layer;
        if (i < 0 || i >= nl || !c.up_has_attn[i]) return DSIM_ERR_INVALID;
        if (c.tap_attn > c.layers_per_block) return DSIM_ERR_INVALID;
        level = nl - 1 - i;
    } else {
        return DSIM_ERR_INVALID;
    }
    const int depth = c.depth_per_level[level] > 0 ? c.depth_per_level[level] : 1;
    if (c.tap_tfm >= depth) return DSIM_ERR_INVALID;
    // spatial side at that level: one downsample per level except after the last
    int side = c.sample_size;
    for (int l = 0; l < level; ++l) side = (side + 1) / 2;        // stride-2 convs: ceil (odd sides)
    const int C = c.block_out_channels[level];
    const int H = c.heads_per_level[level] > 0 ? c.heads_per_level[level] : c.num_heads;
    *tokens = side * side;
    *heads = H;
    *hd = C / H;
    return DSIM_OK;
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

int dsim_unet_create(const dsim_unet_cfg* cfg, dsim_unet** out) {
    if (!cfg || !out) return DSIM_ERR_INVALID;
    if (cfg->n_levels < 1 || cfg->n_levels > DSIM_MAX_LEVELS) return DSIM_ERR_INVALID;
    int t, hh, d;
    CK(tap_geometry(*cfg, &t, &hh, &d));
    return handle_create(cfg, out);
}

void dsim_unet_destroy(dsim_unet* h) { delete h; }

int dsim_unet_load_weight(dsim_unet* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim) {
    return handle_load(h, key, dev_ptr, dtype, shape, ndim);
}

int dsim_unet_finalize(dsim_unet* h, void* stream) {
    if (!h) return DSIM_ERR_INVALID;
    if (h->finalized) return DSIM_ERR_STATE;
    hipStream_t s = (hipStream_t)stream;
    CK(pack_all(h, s));
    const int ted = h->cfg.block_out_channels[0] * 4;
    const int addin = h->cfg.addition_embed ? h->cfg.pooled_dim + 6 * h->cfg.addition_time_embed_dim : 0;
    CK(h->dalloc((size_t)2 * ted * 4, (void**)&h->temb));
    CK(h->dalloc((size_t)(h->cfg.block_out_channels[0] + 5 * ted + addin + 64) * 4, (void**)&h->tscratch));
    // conv1.bias_eff / bias_eff2 (conv1.bias + time_emb_proj(silu(temb)) for the even / odd CFG half) are
    // filled by set_timestep / set_conditioning
    std::vector<std::string> res;
    for (auto& kv : h->pk)
        if (ends_with(kv.first, "time_emb_proj.weight")) res.push_back(kv.first);
    for (auto& k : res) {
        const std::string p = k.substr(0, k.size() - strlen("time_emb_proj.weight"));
        for (const char* suffix : {"conv1.bias_eff", "conv1.bias_eff2"}) {
            Packed P;
            P.rows = h->pk[k].rows; P.cols = 1;
            CK(h->dalloc((size_t)P.rows * 4, &P.p));
            h->pk[p + suffix] = P;
        }
    }
    // fused feed-forward (rowres.hip): one weight stream per transformer block of a width the kernel covers (16-bit modes only)
    if (h->dt != DSIM_F32) {
        std::vector<std::string> ffs;
        for (auto& kv : h->pk)
            if (ends_with(kv.first, "ff.net.0.proj.weight") && ff_stream_bytes(kv.second.cols)) ffs.push_back(kv.first);
        for (auto& k : ffs) {
            const std::string b = k.substr(0, k.size() - strlen("ff.net.0.proj.weight"));
            const Packed* w2 = h->find(b + "ff.net.2.weight");
            if (!w2) return DSIM_ERR_MISSING_WEIGHT;
            const int C = h->pk[k].cols;
            Packed P;
            P.rows = 1; P.cols = C; P.bytes = ff_stream_bytes(C);
            CK(h->dalloc(P.bytes, &P.p));
            CK(pack_ff_stream(h->pk[k].p, w2->p, P.p, C, s));
            h->pk[b + "ff.stream"] = P;
        }
        // LayerNorm-fronted projections of the same blocks: norm1 -> to_q|to_k|to_v and norm2 -> attn2.to_q; and the
        // GroupNorm-fronted proj_in of their Transformer2DModel (N <= K: the GroupNorm form's bound)
        std::vector<std::pair<std::string, std::string>> lps;
        for (auto& kv : h->pk) {
            if (ends_with(kv.first, "proj_in.weight") && kv.second.rows <= kv.second.cols && rowlin_stream_bytes(kv.second.cols, kv.second.rows))
                lps.push_back({kv.first, kv.first.substr(0, kv.first.size() - strlen("weight")) + "stream"});
            if (ends_with(kv.first, "attn1.qkv") && rowlin_stream_bytes(kv.second.cols, kv.second.rows))
                lps.push_back({kv.first, kv.first + ".stream"});
            if (ends_with(kv.first, "attn2.to_q.weight") && rowlin_stream_bytes(kv.second.cols, kv.second.rows))
                lps.push_back({kv.first, kv.first.substr(0, kv.first.size() - strlen("weight")) + "stream"});
        }
        for (auto& kn : lps) {
            const Packed& W = h->pk[kn.first];
            Packed P;
            P.rows = W.rows; P.cols = W.cols; P.bytes = rowlin_stream_bytes(W.cols, W.rows);
            CK(h->dalloc(P.bytes, &P.p));
            CK(pack_rowlin_stream(W.p, P.p, W.cols, W.rows, s));
            h->pk[kn.second] = P;
        }
    }
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    h->raw.clear();
    h->finalized = true;
    // make sure every parameter up to the tap exists: dry walk
    Arena ar;
    Walk w{h, &ar, s, 2, false};
    w.taps = cfg_taps(h->cfg);
    const int st = w.go(nullptr, nullptr, 0.f, 0.f, nullptr);
    if (st != DSIM_OK) { h->finalized = false; return st; }
    return DSIM_OK;
}

static int set_cond(dsim_unet* h, int t, const float* text_embeds, const float* time_ids, hipStream_t s) {
    const dsim_unet_cfg& c = h->cfg;
    const int ch0 = c.block_out_channels[0], ted = ch0 * 4;
    const bool add = c.addition_embed != 0;
    if (add && (!text_embeds || !time_ids)) return DSIM_ERR_INVALID;
    float* emb = h->tscratch;              // [ch0]
    float* h1 = emb + ch0;                 // [ted]
    float* tp = h1 + ted;                  // [ted] per-resnet projection
    float* base = tp + ted;                // [ted] time_embedding(t)
    float* a1 = base + ted;                // [ted]
    float* aug = a1 + ted;                 // [ted]
    float* ain = aug + ted;                // [pooled + 6*atd]
    const Packed* w1 = h->find("time_embedding.linear_1.weight");
    const Packed* b1 = h->find("time_embedding.linear_1.bias");
    const Packed* w2 = h->find("time_embedding.linear_2.weight");
    const Packed* b2 = h->find("time_embedding.linear_2.bias");
    if (!w1 || !b1 || !w2 || !b2) return DSIM_ERR_MISSING_WEIGHT;
    CK(timestep_sincos(emb, ch0, t, s));
    CK(gemv_f32(w1->p, DSIM_F32, b1->p, DSIM_F32, emb, h1, ted, ch0, 0, s));
    CK(gemv_f32(w2->p, DSIM_F32, b2->p, DSIM_F32, h1, base, ted, ted, 1, s));
    for (int half = 0; half < 2; ++half) {
        float* temb = h->temb + (size_t)half * ted;
        if (add) {
            // UNet2DConditionModel "text_time": cat(text_embeds, Timesteps(time_ids.flatten())) -> add_embedding
            const Packed* aw1 = h->find("add_embedding.linear_1.weight");
            const Packed* ab1 = h->find("add_embedding.linear_1.bias");
            const Packed* aw2 = h->find("add_embedding.linear_2.weight");
            const Packed* ab2 = h->find("add_embedding.linear_2.bias");
            if (!aw1 || !ab1 || !aw2 || !ab2) return DSIM_ERR_MISSING_WEIGHT;
            const int P = c.pooled_dim, atd = c.addition_time_embed_dim, nin = P + 6 * atd;
            DSIM_HIP_CHECK(hipMemcpyAsync(ain, text_embeds + (size_t)half * P, (size_t)P * 4, hipMemcpyDeviceToDevice, s));
            CK(sincos_values(ain + P, atd, time_ids + (size_t)half * 6, 6, s));
            CK(gemv_f32(aw1->p, DSIM_F32, ab1->p, DSIM_F32, ain, a1, ted, nin, 0, s));
            CK(gemv_f32(aw2->p, DSIM_F32, ab2->p, DSIM_F32, a1, aug, ted, ted, 1, s));
            CK(add_vectors_f32(base, aug, temb, ted, s));
        } else {
            DSIM_HIP_CHECK(hipMemcpyAsync(temb, base, (size_t)ted * 4, hipMemcpyDeviceToDevice, s));
        }
        for (auto& kv : h->pk) {
            if (!ends_with(kv.first, "time_emb_proj.weight")) continue;
            const std::string p = kv.first.substr(0, kv.first.size() - strlen("time_emb_proj.weight"));
            const Packed* tb = h->find(p + "time_emb_proj.bias");
            const Packed* cb = h->find(p + "conv1.bias");
            const Packed* eff = h->find(p + (half ? "conv1.bias_eff2" : "conv1.bias_eff"));
            if (!tb || !cb || !eff) return DSIM_ERR_MISSING_WEIGHT;
            const int n = kv.second.rows;
            if (n > ted) return DSIM_ERR_INVALID;
            CK(gemv_f32(kv.second.p, DSIM_F32, tb->p, DSIM_F32, temb, tp, n, ted, 1, s));
            CK(add_vectors_f32((const float*)cb->p, tp, (float*)eff->p, n, s));
        }
    }
    h->two_temb = add;
    h->timestep = t;
    return DSIM_OK;
}

int dsim_unet_set_timestep(dsim_unet* h, int t, void* stream) {
    if (!h || t < 0) return DSIM_ERR_INVALID;
    if (!h->finalized) return DSIM_ERR_STATE;
    if (h->cfg.addition_embed) return DSIM_ERR_STATE;       // SDXL graphs need set_conditioning
    return set_cond(h, t, nullptr, nullptr, (hipStream_t)stream);
}

int dsim_unet_set_conditioning(dsim_unet* h, int t, const float* text_embeds, const float* time_ids, void* stream) {
    if (!h || t < 0) return DSIM_ERR_INVALID;
    if (!h->finalized) return DSIM_ERR_STATE;
    return set_cond(h, t, text_embeds, time_ids, (hipStream_t)stream);
}

// the handle's cfg with its tap fields set to `t` (tap_geometry's input for a tap other than the handle's own)
static dsim_unet_cfg cfg_at(const dsim_unet_cfg& c, int block, int layer, int attn, int tfm) {
    dsim_unet_cfg r = c;
    r.tap_block = block; r.tap_layer = layer; r.tap_attn = attn; r.tap_tfm = tfm;
    return r;
}

// The taps of one sweep, checked: tap_geometry accepts each, and no two name the same attention once -1 (the last) is resolved
// and the mid block's unused fields are ignored.  out_bytes: the largest q / k / v tensor of n_images.
static int check_taps(const dsim_unet* h, int n_images, int n_taps, const dsim_tap* taps, std::vector<TapReq>* out,
                      size_t* out_bytes) {
    if (n_taps < 1 || !taps) return DSIM_ERR_INVALID;
    const dsim_unet_cfg& c = h->cfg;
    std::vector<std::array<int, 4>> seen;
    out->clear();
    *out_bytes = 0;
    for (int i = 0; i < n_taps; ++i) {
        const dsim_tap& t = taps[i];
        int n, hh, d;
        CK(tap_geometry(cfg_at(c, t.block, t.layer, t.attn, t.tfm), &n, &hh, &d));
        const size_t b = (size_t)2 * n_images * n * hh * d * dtype_size(h->dt);
        if (b > *out_bytes) *out_bytes = b;
        const int nl = c.n_levels;
        const int level = t.block == DSIM_TAP_DOWN ? t.layer : (t.block == DSIM_TAP_MID ? nl - 1 : nl - 1 - t.layer);
        const int depth = c.depth_per_level[level] > 0 ? c.depth_per_level[level] : 1;
        const int nattn = t.block == DSIM_TAP_DOWN ? c.layers_per_block : c.layers_per_block + 1;
        const std::array<int, 4> key = {t.block, t.block == DSIM_TAP_MID ? 0 : t.layer,
                                        t.block == DSIM_TAP_MID ? 0 : (t.attn < 0 ? nattn - 1 : t.attn), t.tfm < 0 ? depth - 1 : t.tfm};
        for (const auto& s2 : seen)
            if (s2 == key) return DSIM_ERR_INVALID;
        seen.push_back(key);
        out->push_back(TapReq{t.block, t.layer, t.attn, t.tfm});
    }
    return DSIM_OK;
}

// dry walk to the deepest of `taps`: peak arena bytes and the largest activation
static int plan_taps(dsim_unet* h, int n_images, const std::vector<TapReq>& taps, size_t* peak, size_t* max_tensor, int n_ctx = 1,
                     bool text = false) {
    Arena ar;
    Walk w{h, &ar, nullptr, 2 * n_images, false};
    w.taps = taps;
    w.n_ctx = n_ctx;
    w.text = text;
    CK(w.go(nullptr, nullptr, 0.f, 0.f, nullptr));
    *peak = ar.peak;
    *max_tensor = w.max_tensor;
    return DSIM_OK;
}

// a context table of n_ctx rows: SD1.5-family handles only.  SDXL's pooled prompt embedding enters the time embedding, which
// reaches every resnet as a per-CFG-half bias: one prompt per call there.
static bool ctx_table_ok(const dsim_unet* h, int n_ctx) {
    return n_ctx == 1 || (n_ctx > 1 && !h->two_temb && !h->cfg.addition_embed);
}

static size_t workspace_bytes(dsim_unet* h, int n_images, int n_ctx, bool text = false) {
    if (!h || !h->finalized || n_images < 1 || !ctx_table_ok(h, n_ctx)) return 0;
    size_t peak, big;
    if (plan_taps(h, n_images, cfg_taps(h->cfg), &peak, &big, n_ctx, text) != DSIM_OK) return 0;
    if (big >= 0x7fffffffull) return 0;      // a >= 2 GiB activation: the batch does not fit one call
    return peak + 256;
}

static size_t taps_workspace_bytes(dsim_unet* h, int n_images, int n_ctx, int n_taps, const dsim_tap* taps) {
    if (!h || !h->finalized || n_images < 1 || !ctx_table_ok(h, n_ctx)) return 0;
    std::vector<TapReq> req;
    size_t out_bytes, peak, big;
    if (check_taps(h, n_images, n_taps, taps, &req, &out_bytes) != DSIM_OK) return 0;
    if (plan_taps(h, n_images, req, &peak, &big, n_ctx) != DSIM_OK) return 0;
    if (big >= 0x7fffffffull || out_bytes >= 0x7fffffffull) return 0;
    return peak + 256;
}

size_t dsim_unet_workspace_bytes(const dsim_unet* hc, int n_images) {
    return workspace_bytes(const_cast<dsim_unet*>(hc), n_images, 1);
}

size_t dsim_unet_ctx_workspace_bytes(const dsim_unet* hc, int n_images, int n_ctx) {
    return workspace_bytes(const_cast<dsim_unet*>(hc), n_images, n_ctx);
}

size_t dsim_unet_text_workspace_bytes(const dsim_unet* hc, int n_images, int n_ctx) {
    return workspace_bytes(const_cast<dsim_unet*>(hc), n_images, n_ctx, true);
}

size_t dsim_unet_taps_workspace_bytes(const dsim_unet* hc, int n_images, int n_taps, const dsim_tap* taps) {
    return taps_workspace_bytes(const_cast<dsim_unet*>(hc), n_images, 1, n_taps, taps);
}

size_t dsim_unet_taps_ctx_workspace_bytes(const dsim_unet* hc, int n_images, int n_ctx, int n_taps, const dsim_tap* taps) {
    return taps_workspace_bytes(const_cast<dsim_unet*>(hc), n_images, n_ctx, n_taps, taps);
}

int dsim_unet_tap_shape(const dsim_unet* h, int* tokens, int* heads, int* head_dim) {
    if (!h || !tokens || !heads || !head_dim) return DSIM_ERR_INVALID;
    return tap_geometry(h->cfg, tokens, heads, head_dim);
}

int dsim_unet_tap_shape_at(const dsim_unet* h, const dsim_tap* tap, int* tokens, int* heads, int* head_dim) {
    if (!h || !tap || !tokens || !heads || !head_dim) return DSIM_ERR_INVALID;
    return tap_geometry(cfg_at(h->cfg, tap->block, tap->layer, tap->attn, tap->tfm), tokens, heads, head_dim);
}

int dsim_unet_set_tap(dsim_unet* h, int tap_block, int tap_layer, int tap_attn, int tap_tfm) {
    if (!h) return DSIM_ERR_INVALID;
    if (!h->finalized) return DSIM_ERR_STATE;
    const dsim_unet_cfg old = h->cfg;
    h->cfg.tap_block = tap_block; h->cfg.tap_layer = tap_layer; h->cfg.tap_attn = tap_attn; h->cfg.tap_tfm = tap_tfm;
    int t, hh, d;
    int st = tap_geometry(h->cfg, &t, &hh, &d);
    if (st == DSIM_OK) {             // every parameter up to the new tap must have been loaded: dry walk
        Arena ar;
        Walk w{h, &ar, nullptr, 2, false};
        w.taps = cfg_taps(h->cfg);
        st = w.go(nullptr, nullptr, 0.f, 0.f, nullptr);
    }
    if (st != DSIM_OK) h->cfg = old;
    return st;
}

int dsim_unet_set_cfg_dedup(dsim_unet* h, int enable) {
    if (!h) return DSIM_ERR_INVALID;
    h->cfg_dedup = enable != 0;
    return DSIM_OK;
}

int dsim_unet_set_fusion(dsim_unet* h, int mask) {
    if (!h || (mask & ~DSIM_FUSE_ALL)) return DSIM_ERR_INVALID;
    h->fusion = mask;
    return DSIM_OK;
}

int dsim_unet_set_sample_size(dsim_unet* h, int side) {
    if (!h || side < 2) return DSIM_ERR_INVALID;          // any side: odd levels take the ceil-div / explicit-size path
    h->cfg.sample_size = side;
    return DSIM_OK;
}

// one walk to the deepest of `taps` (their outputs set), every check before the first launch
static int run_taps(dsim_unet* h, const float* latents, const float* noise, float sqrt_abar, float sqrt_1m_abar, const float* ctx,
                    int n_images, const std::vector<TapReq>& taps, void* workspace, size_t workspace_bytes, void* stream, int n_ctx,
                    const int32_t* ctx_index, void* text_xq = nullptr, void* text_xkv = nullptr) {
    bool tapped = false;
    const bool text = text_xq != nullptr;
    CK(run_in_workspace(
        workspace, workspace_bytes,
        [&](size_t* peak) {
            size_t big;
            return plan_taps(h, n_images, taps, peak, &big, n_ctx, text);
        },
        [&](Arena& ar) {
            Walk w{h, &ar, (hipStream_t)stream, 2 * n_images, true};
            w.taps = taps;
            w.n_ctx = n_ctx;
            w.ctx_index = ctx_index;
            w.text = text; w.text_xq = text_xq; w.text_xkv = text_xkv;
            const int st = w.go(latents, noise, sqrt_abar, sqrt_1m_abar, ctx);
            tapped = w.tapped;
            return st;
        }));
    return tapped ? DSIM_OK : DSIM_ERR_INVALID;        // (a walk that reached no tap is an invalid tap here; dit_run calls it a workspace error)
}

// What the four dsim_unet_qkv* entry points are: the argument, context-table and state checks, the tap list, one walk.  own_tap: the
// handle's own tap (n_taps / taps unused; q, k, v name one tensor each).
static int qkv_call(dsim_unet* h, const float* latents, const float* noise, float sqrt_abar, float sqrt_1m_abar, const float* ctx,
                    int n_ctx, const int32_t* ctx_index, int n_images, bool own_tap, int n_taps, const dsim_tap* taps, void* const* q,
                    void* const* k, void* const* v, void* workspace, size_t workspace_bytes, void* stream, void* text_xq = nullptr,
                    void* text_xkv = nullptr) {
    if (!h || !latents || !noise || !ctx || !q || !k || !v || !workspace || n_images < 1) return DSIM_ERR_INVALID;
    if (own_tap && (!*q || !*k || !*v)) return DSIM_ERR_INVALID;
    if (n_ctx < 1 || (n_ctx > 1 && !ctx_index) || !ctx_table_ok(h, n_ctx)) return DSIM_ERR_INVALID;
    if (!h->finalized || h->timestep < 0) return DSIM_ERR_STATE;
    std::vector<TapReq> req = cfg_taps(h->cfg);
    size_t out_bytes;
    if (!own_tap) CK(check_taps(h, n_images, n_taps, taps, &req, &out_bytes));
    for (size_t i = 0; i < req.size(); ++i) {
        if (!q[i] || !k[i] || !v[i]) return DSIM_ERR_INVALID;
        req[i].q = q[i]; req[i].k = k[i]; req[i].v = v[i];
    }
    return run_taps(h, latents, noise, sqrt_abar, sqrt_1m_abar, ctx, n_images, req, workspace, workspace_bytes, stream, n_ctx,
                    n_ctx > 1 ? ctx_index : nullptr, text_xq, text_xkv);
}

int dsim_unet_qkv(dsim_unet* h, const float* latents, const float* noise, float sqrt_abar, float sqrt_1m_abar,
                  const float* ctx, int n_images, void* q, void* k, void* v, void* workspace, size_t workspace_bytes,
                  void* stream) {
    return qkv_call(h, latents, noise, sqrt_abar, sqrt_1m_abar, ctx, 1, nullptr, n_images, true, 0, nullptr, &q, &k, &v, workspace,
                    workspace_bytes, stream);
}

int dsim_unet_qkv_taps(dsim_unet* h, const float* latents, const float* noise, float sqrt_abar, float sqrt_1m_abar, const float* ctx,
                       int n_images, int n_taps, const dsim_tap* taps, void* const* q, void* const* k, void* const* v, void* workspace,
                       size_t workspace_bytes, void* stream) {
    return qkv_call(h, latents, noise, sqrt_abar, sqrt_1m_abar, ctx, 1, nullptr, n_images, false, n_taps, taps, q, k, v, workspace,
                    workspace_bytes, stream);
}

int dsim_unet_qkv_ctx(dsim_unet* h, const float* latents, const float* noise, float sqrt_abar, float sqrt_1m_abar, const float* ctx,
                      int n_ctx, const int32_t* ctx_index, int n_images, void* q, void* k, void* v, void* workspace,
                      size_t workspace_bytes, void* stream) {
    return qkv_call(h, latents, noise, sqrt_abar, sqrt_1m_abar, ctx, n_ctx, ctx_index, n_images, true, 0, nullptr, &q, &k, &v, workspace,
                    workspace_bytes, stream);
}

int dsim_unet_qkv_text(dsim_unet* h, const float* latents, const float* noise, float sqrt_abar, float sqrt_1m_abar, const float* ctx,
                       int n_ctx, const int32_t* ctx_index, int n_images, void* q, void* k, void* v, void* xq, void* xkv, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (!xq || !xkv) return DSIM_ERR_INVALID;
    return qkv_call(h, latents, noise, sqrt_abar, sqrt_1m_abar, ctx, n_ctx, ctx_index, n_images, true, 0, nullptr, &q, &k, &v, workspace,
                    workspace_bytes, stream, xq, xkv);
}

int dsim_unet_qkv_taps_ctx(dsim_unet* h, const float* latents, const float* noise, float sqrt_abar, float sqrt_1m_abar, const float* ctx,
                           int n_ctx, const int32_t* ctx_index, int n_images, int n_taps, const dsim_tap* taps, void* const* q,
                           void* const* k, void* const* v, void* workspace, size_t workspace_bytes, void* stream) {
    return qkv_call(h, latents, noise, sqrt_abar, sqrt_1m_abar, ctx, n_ctx, ctx_index, n_images, false, n_taps, taps, q, k, v, workspace,
                    workspace_bytes, stream);
}

int dsim_unet_profile(dsim_unet* h, int enable) { return prof_enable(h, enable); }
int dsim_unet_profile_count(const dsim_unet* h) { return prof_count(h); }
int dsim_unet_profile_get(dsim_unet* h, int i, char* name, int name_cap, double* flops, double* bytes, double* ms) {
    return prof_get(h, i, name, name_cap, flops, bytes, ms);
}

}  // extern "C"
