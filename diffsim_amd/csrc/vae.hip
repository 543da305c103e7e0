// VAE encoder executor (AutoencoderKL.encode) and its C ABI -- SURVEY.md section 8f row 1.
//
// Replaces `pipe.vae.encode(image)` of the reference (diffsim/diffsim.py:92-96).  The arithmetic
// lives in un-vendored diffusers; it is restated from SURVEY.md Appendix A item 11:
//   conv_in 3->C0 | 4 x DownEncoderBlock2D (2 ResnetBlock2D without time embedding, GroupNorm eps 1e-6;
//   downsample = pad(0,1,0,1) + 3x3 stride-2 conv) | mid: resnet, 1-head attention with GroupNorm
//   and residual, resnet | GroupNorm + SiLU + conv_out -> quant_conv 1x1 -> (mean, logvar).
// Kernel reuse: every conv is the implicit-GEMM MFMA kernel (the stride-2 form with pad = 0),
// GroupNorm(+SiLU) is the two-pass HBM-bound kernel, conv_in is the direct small-K kernel.  The
// mid-block attention has one 512-wide head, too wide for the register-resident flash kernel, so
// it runs as three GEMMs per image around a row-softmax: S = q k^T, P = softmax(S/sqrt(C)),
// O = P v (+ b_v as a column bias: rows of P sum to one).  quant_conv is folded into conv_out at
// finalize (both are linear): W' = Wq Wco, b' = Wq bco + bq.
// Sampling z = mean + exp(0.5*clamp(logvar)) * eps stays on the host side (it consumes the
// caller's CPU generator in the reference's draw order).
#include <string>

#include "common.h"
#include "store.h"

using namespace dsim;

constexpr int VAE_VREP = 16;          // copies of the mid-block attention's to_v weight (finalize): images per batched v^T launch

struct dsim_vae : WeightStore {
    dsim_vae_cfg cfg;
};

namespace {

// W'[o][k] = sum_c Wq[o][c] * Wco[c][k]   (Wco packed [Cm][K] compute dtype; Wq f32 [Cm][Cm])
template <typename T>
__global__ void fold_quant_kernel(const float* __restrict__ wq, const T* __restrict__ wco, T* __restrict__ out, int Cm,
                                  int K) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, o = blockIdx.y;
    if (k >= K) return;
    float acc = 0.f;
    for (int c = 0; c < Cm; ++c) acc = fmaf(wq[o * Cm + c], (float)wco[(size_t)c * K + k], acc);
    out[(size_t)o * K + k] = (T)acc;
}
__global__ void fold_quant_bias_kernel(const float* wq, const float* bco, const float* bq, float* out, int Cm) {
    const int o = threadIdx.x;
    if (o >= Cm) return;
    float acc = bq[o];
    for (int c = 0; c < Cm; ++c) acc = fmaf(wq[o * Cm + c], bco[c], acc);
    out[o] = acc;
}
// token-major [n][hw][C] compute dtype -> f32 NCHW [n][C][hw]
template <typename T>
__global__ void to_nchw_f32_kernel(const T* __restrict__ x, float* __restrict__ out, int HW, int Cc, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % Cc);
    const size_t t = i / Cc;
    const int p = (int)(t % HW);
    const size_t n = t / HW;
    out[(n * Cc + c) * HW + p] = (float)x[i];
}

struct VWalk : WalkBase<dsim_vae> {
    const int n;            // images
    void* gn_scratch = nullptr;
    VWalk(dsim_vae* h, Arena* ar, hipStream_t s, int n, bool run) : WalkBase(h, ar, s, run), n(n) {}

    int linear(const void* a, int K, const void* w, const float* bias, const void* residual, void* out, int M, int N) {
        GemmArgs g = linear_args(a, K, w, bias, residual, out, M, N);
        return gemm(g);
    }
    // The 128 x 128 level (one image = 64 ... 128 of the 256-row tiles): its convs ask for those tiles at EVERY batch size
    // (GemmArgs.force_big), so that the statistics can come from the epilogue there as well -- a single image then runs that level's
    // convs on half the chip (+0.1 ms of a ~12 ms encode), every pair or chunk as before
    static int big_tiles(int hw, int Cout) { return hw >= 128 * 128 && hw % 256 == 0 && Cout % 256 == 0; }
    // GroupNorm statistics of a conv's output from its epilogue (GemmArgs.gn_part): can the conv g produce them?  Where ONE image alone
    // fills the chip's 256-row tiles (the 512 x 512 and 256 x 256 levels: the same tiles at every batch size, so the numbers do not
    // depend on the batch; asked with the geometry of a single image).  Leaves g.force_big as the answer needs it.
    bool epilogue_stats(GemmArgs& g) const {
        const int hw = g.Hout * g.Wout, cpg = g.N / h->cfg.norm_num_groups;
        g.force_big = big_tiles(hw, g.N);
        GemmArgs one = g;
        one.M = hw;
        if (h->cfg.norm_num_groups == 32 && g.N % 32 == 0 && (cpg == 4 || cpg == 8 || cpg == 16) && gemm_gn_stats_tile(one, h->dt)) return true;
        g.force_big = 0;
        return false;
    }
    // the partial-sum buffer of those statistics for B images of hw pixels x C channels
    float* alloc_stats(int B, int hw, int C) { return (float*)ar->alloc((size_t)B * (hw / 64) * (C / 4) * 2 * sizeof(float)); }
    static void stats_to(GemmArgs& g, float* part) { g.gn_part = part; g.gn_hw = g.Hout * g.Wout; }

    // `stats` receives the partial buffer for the GroupNorm that consumes the output (null: that GroupNorm runs its own pass)
    int conv3(const Act& x, const Packed* w, const float* bias, const void* residual, void* out, int Cout, int stride, int pad,
              float** stats = nullptr) {
        GemmArgs g = conv3_args(x, w->p, bias, residual, out, Cout, stride, 0, pad);
        if (stats) {
            *stats = epilogue_stats(g) ? alloc_stats(x.B, g.Hout * g.Wout, Cout) : nullptr;
            if (*stats) stats_to(g, *stats);
        }
        return gemm(g);
    }
    int gn(const Act& x, const Packed* g, const Packed* b, void* out, int silu, const float* stats = nullptr) {
        const int HW = x.H * x.W, groups = h->cfg.norm_num_groups;
        const float *gw = (const float*)g->p, *gb = (const float*)b->p;
        return launch([&] { return gn_rec(x.B, HW, x.C, 0, groups, stats != nullptr); },
                      [&] {
                          return stats ? launch_groupnorm_pre(x.p, x.C, gw, gb, out, x.B, HW, groups, 1e-6f, silu, h->dt, gn_scratch, stats,
                                                              HW / 64, s)
                                       : launch_groupnorm(x.p, x.C, nullptr, 0, gw, gb, out, x.B, HW, groups, 1e-6f, silu, h->dt, gn_scratch, s);
                      });
    }

    // in_stats: epilogue statistics of x (from the conv that produced it) for norm1; out_stats: receives those of this block's output
    int resnet(const std::string& p, const Act& x, int Cout, Act* out, const float* in_stats = nullptr, float** out_stats = nullptr) {
        const int Cin = x.C, B = x.B, H = x.H, W = x.W, M = x.rows();
        WGET(n1w, p + "norm1.weight"); WGET(n1b, p + "norm1.bias");
        WGET(c1w, p + "conv1.weight"); WGET(c1b, p + "conv1.bias");
        WGET(n2w, p + "norm2.weight"); WGET(n2b, p + "norm2.bias");
        WGET(c2w, p + "conv2.weight"); WGET(c2b, p + "conv2.bias");
        *out = act(B, H, W, Cout);
        // conv2 + residual, but for its input and residual (known below).  Its epilogue statistics (for the next block's norm1) outlive
        // this block's scratch: their buffer is allocated before the mark
        GemmArgs c2 = conv3_args(Act{nullptr, Cout, H, W, B}, c2w->p, (const float*)c2b->p, x.p, out->p, Cout, 1, 0, 1);
        float* ostat = out_stats && epilogue_stats(c2) ? alloc_stats(B, H * W, Cout) : nullptr;
        if (ostat) stats_to(c2, ostat);
        const size_t mk = ar->mark();
        const Act t1 = act(B, H, W, Cin);
        CK(gn(x, n1w, n1b, t1.p, 1, in_stats));
        const Act t2 = act(B, H, W, Cout);
        float* st2 = nullptr;
        CK(conv3(t1, c1w, (const float*)c1b->p, nullptr, t2.p, Cout, 1, 1, &st2));
        Act t3{t1.p, Cout, H, W, B};
        if (Cout > Cin) t3.p = alloc_act((size_t)M * Cout);
        CK(gn(t2, n2w, n2b, t3.p, 1, st2));
        c2.A0 = t3.p;
        if (Cin != Cout) {
            WGET(scw, p + "conv_shortcut.weight"); WGET(scb, p + "conv_shortcut.bias");
            void* sc = t2.p;                                   // t2 is dead after norm2
            CK(linear(x.p, Cin, scw->p, (const float*)scb->p, nullptr, sc, M, Cout));
            c2.residual = sc;
        }
        CK(gemm(c2));
        if (out_stats) *out_stats = ostat;
        ar->release(mk);
        return DSIM_OK;
    }

    int attention(const std::string& p, const Act& x, Act* out) {
        const int C = x.C, N = x.H * x.W, M = x.rows();
        WGET(gw, p + "group_norm.weight"); WGET(gb, p + "group_norm.bias");
        WGET(wq, p + "to_q.weight"); WGET(bq, p + "to_q.bias");
        WGET(wk, p + "to_k.weight"); WGET(bk, p + "to_k.bias");
        WGET(wv, p + "to_v.weight"); WGET(bv, p + "to_v.bias");
        WGET(wo, p + "to_out.0.weight"); WGET(bo, p + "to_out.0.bias");
        *out = act(n, x.H, x.W, C);
        const size_t mk = ar->mark();
        char* t = (char*)alloc_act((size_t)M * C);
        CK(gn(x, gw, gb, t, 0));
        char* q = (char*)alloc_act((size_t)M * C);
        char* k = (char*)alloc_act((size_t)M * C);
        char* o = (char*)alloc_act((size_t)M * C);
        CK(linear(t, C, wq->p, (const float*)bq->p, nullptr, q, M, C));
        CK(linear(t, C, wk->p, (const float*)bk->p, nullptr, k, M, C));
        // Images per group: the score matrices of a whole group come from ONE batched launch each way (GemmArgs.wb_rows: row block i
        // multiplies image i's k / v^T), so the 32-tile P v of a single 4096-token image no longer runs as 16 x n quarter-chip
        // launches; same tiles' arithmetic bit for bit (gemm_skinny_kernel == gemm_kernel, asserted in the tests), so an image's
        // moments do not depend on its group.  Token counts that are not whole 256-row tiles keep one image per launch.
        int grp = 1;
        if (N % 256 == 0) {
            const size_t lim = 0x7fffffffull / ((size_t)N * N * es());
            grp = (int)std::min<size_t>((size_t)n, lim < 1 ? 1 : lim);
        }
        void* sc = alloc_act((size_t)grp * N * N);             // the group's score matrices
        char* vT = (char*)alloc_act((size_t)grp * C * N);
        const size_t img = (size_t)N * C * es();
        for (int i0 = 0; i0 < n; i0 += grp) {
            const int gi = std::min(grp, n - i0);
            const Packed* wrep = h->find(p + "to_v.weight_rep");
            for (int i = 0; i < gi;) {                                                                // v^T = Wv x^T
                const int nb = (wrep && C % 256 == 0) ? std::min(gi - i, VAE_VREP) : 1;
                GemmArgs gv = linear_args(nb > 1 ? wrep->p : wv->p, C, t + (i0 + i) * img, nullptr, nullptr, vT + i * img, nb * C, N);
                if (nb > 1) { gv.wb_rows = C; gv.wb_stride = (unsigned)img; }
                CK(gemm(gv));
                i += nb;
            }
            GemmArgs g = linear_args(q + i0 * img, C, k + i0 * img, nullptr, nullptr, sc, gi * N, N);
            g.wb_rows = N; g.wb_stride = (unsigned)img;
            CK(gemm(g));                                                                              // S = q k^T
            CK(launch([&] { return rec(std::string("softmax_rows_") + dtn() + "|N" + std::to_string(N), 0.0,
                                       2.0 * gi * N * (double)N * es()); },
                      [&] { return launch_softmax_rows(sc, sc, gi * N, N, 1.0f / sqrtf((float)C), h->dt, s); }));
            GemmArgs o2 = linear_args(sc, N, vT, (const float*)bv->p, nullptr, o + i0 * img, gi * N, C);
            o2.wb_rows = N; o2.wb_stride = (unsigned)img;
            CK(gemm(o2));                                                                             // O = P v + b_v
        }
        CK(linear(o, C, wo->p, (const float*)bo->p, x.p, out->p, M, C));
        ar->release(mk);
        return DSIM_OK;
    }

    int go(const float* images, int S, float* moments) {
        const dsim_vae_cfg& c = h->cfg;
        const int nl = c.n_levels, ch0 = c.block_out_channels[0];
        gn_scratch = ar->alloc(groupnorm_scratch_bytes(n, c.norm_num_groups));
        WGET(ciw, "encoder.conv_in.weight"); WGET(cib, "encoder.conv_in.bias");
        Act x = act(n, S, S, ch0);
        float* xstat = nullptr;                 // epilogue statistics of x, when its producer made them
        const bool rows = conv_in_rows_applies(c.in_channels, S, ch0);
        if (rows && h->dt != DSIM_F32 && c.norm_num_groups == 32) xstat = alloc_stats(n, S * S, ch0);      // (one 4-channel quad per group at 128 channels)
        CK(launch([&] { return rec(rows ? "conv_in_rows" : "prep_conv_in", 2.0 * n * S * S * (double)ch0 * 9 * c.in_channels,
                                   (double)n * S * S * (ch0 * es() + c.in_channels * 4.0)); },
                  [&] {
                      return rows ? conv_in_rows(images, (const float*)ciw->p, (const float*)cib->p, x.p, h->dt, n, S, xstat, s)
                                  : prep_conv_in(images, nullptr, 1.f, 0.f, (const float*)ciw->p, (const float*)cib->p, x.p, h->dt, n,
                                                 c.in_channels, S, ch0, 1, s);
                  }));
        for (int i = 0; i < nl; ++i) {
            const int co = c.block_out_channels[i];
            const std::string bp = "encoder.down_blocks." + std::to_string(i) + ".";
            for (int j = 0; j < c.layers_per_block; ++j) {
                Act r;
                float* rstat = nullptr;
                // (the last resnet of a level feeds the downsample conv, not a GroupNorm: no statistics asked of it)
                CK(resnet(bp + "resnets." + std::to_string(j) + ".", x, co, &r, xstat, j + 1 < c.layers_per_block ? &rstat : nullptr));
                x = r;
                xstat = rstat;
            }
            if (i != nl - 1) {
                WGET(dw, bp + "downsamplers.0.conv.weight"); WGET(db, bp + "downsamplers.0.conv.bias");
                const Act d = act(n, x.H / 2, x.W / 2, co);
                CK(conv3(x, dw, (const float*)db->p, nullptr, d.p, co, 2, 0, &xstat));
                x = d;
            } else {
                xstat = nullptr;
            }
        }
        {
            const int cm = c.block_out_channels[nl - 1];
            Act r;
            CK(resnet("encoder.mid_block.resnets.0.", x, cm, &r)); x = r;
            CK(attention("encoder.mid_block.attentions.0.", x, &r)); x = r;
            CK(resnet("encoder.mid_block.resnets.1.", x, cm, &r)); x = r;
        }
        WGET(nw, "encoder.conv_norm_out.weight"); WGET(nb, "encoder.conv_norm_out.bias");
        WGET(cow, "encoder.conv_out_folded.weight"); WGET(cob, "encoder.conv_out_folded.bias");
        const int Cm = 2 * c.latent_channels;
        const Act t = act(n, x.H, x.W, x.C);
        CK(gn(x, nw, nb, t.p, 1));
        const Act mo = act(n, x.H, x.W, Cm);
        CK(conv3(t, cow, (const float*)cob->p, nullptr, mo.p, Cm, 1, 1));
        CK(launch([&] { return to_nchw_f32(mo.p, moments, n, x.H * x.W, Cm, h->dt, s); }));
        return DSIM_OK;
    }
};

}  // namespace

namespace dsim {
int to_nchw_f32(const void* x, float* out, int n, int HW, int C, int dtype, hipStream_t s) {
    return by_dtype(dtype, [&](auto e) {
        typedef typename decltype(e)::type T;
        const size_t total = (size_t)n * HW * C;
        hipLaunchKernelGGL(to_nchw_f32_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const T*)x, out, HW, C, total);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}
int fold_quant(const float* wq, const void* wco, const float* bco, const float* bq, void* out_w, float* out_b, int Cm, int K, int dtype,
               hipStream_t s) {
    // the bias kernel is one workgroup with a thread per output row: sized from Cm (it was 64 threads whatever Cm, rows past 64 unwritten)
    if (Cm < 1 || Cm > 65535 || K < 1 || (out_b && Cm > 1024)) return DSIM_ERR_INVALID;
    if (out_w)
        CK(by_dtype(dtype, [&](auto e) {
            typedef typename decltype(e)::type T;
            hipLaunchKernelGGL(fold_quant_kernel<T>, dim3((K + 255) / 256, Cm), dim3(256), 0, s, wq, (const T*)wco, (T*)out_w, Cm, K);
            DSIM_HIP_CHECK(hipGetLastError());
            return DSIM_OK;
        }));
    if (out_b) {
        hipLaunchKernelGGL(fold_quant_bias_kernel, dim3(1), dim3((Cm + 63) / 64 * 64), 0, s, wq, bco, bq, out_b, Cm);
        DSIM_HIP_CHECK(hipGetLastError());
    }
    return DSIM_OK;
}
}  // namespace dsim

extern "C" {

int dsim_vae_create(const dsim_vae_cfg* cfg, dsim_vae** out) {
    if (!cfg || !out) return DSIM_ERR_INVALID;
    if (cfg->n_levels < 1 || cfg->n_levels > DSIM_MAX_LEVELS) return DSIM_ERR_INVALID;
    return handle_create(cfg, out);
}

void dsim_vae_destroy(dsim_vae* h) { delete h; }

int dsim_vae_load_weight(dsim_vae* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim) {
    return handle_load(h, key, dev_ptr, dtype, shape, ndim);
}

int dsim_vae_finalize(dsim_vae* h, void* stream) {
    if (!h) return DSIM_ERR_INVALID;
    if (h->finalized) return DSIM_ERR_STATE;
    hipStream_t s = (hipStream_t)stream;
    CK(pack_all(h, s));
    // fold quant_conv (1x1, linear) into conv_out
    const Packed* cow = h->find("encoder.conv_out.weight");
    const Packed* cob = h->find("encoder.conv_out.bias");
    const Packed* qw = h->find("quant_conv.weight");
    const Packed* qb = h->find("quant_conv.bias");
    if (!cow || !cob || !qw || !qb) return DSIM_ERR_MISSING_WEIGHT;
    const int Cm = cow->rows, K = cow->cols;
    // quant_conv.weight was packed as a GEMM weight in the compute dtype; the fold wants it in f32
    float* wq32 = nullptr;
    CK(h->dalloc((size_t)Cm * Cm * 4, (void**)&wq32));
    auto it = h->raw.find("quant_conv.weight");
    if (it == h->raw.end()) return DSIM_ERR_MISSING_WEIGHT;
    CK(pack_vector(it->second.p, it->second.dtype, wq32, Cm * Cm, 0, s));
    Packed fw, fb;
    fw.rows = Cm; fw.cols = K;
    CK(h->dalloc((size_t)Cm * K * dtype_size(h->dt), &fw.p));
    CK(h->dalloc((size_t)Cm * 4, &fb.p));
    fb.rows = Cm; fb.cols = 1;
    CK(fold_quant(wq32, cow->p, (const float*)cob->p, (const float*)qb->p, fw.p, (float*)fb.p, Cm, K, h->dt, s));
    h->pk["encoder.conv_out_folded.weight"] = fw;
    h->pk["encoder.conv_out_folded.bias"] = fb;
    // the mid-block attention's to_v weight, VAE_VREP copies back to back: v^T = Wv x^T of a whole group of images is then ONE launch
    // whose row block i (= copy i of Wv) multiplies image i's tokens (GemmArgs.wb_rows)
    if (const Packed* wv = h->find("encoder.mid_block.attentions.0.to_v.weight")) {
        const size_t one = (size_t)wv->rows * wv->cols * dtype_size(h->dt);
        Packed rep;
        rep.rows = wv->rows * VAE_VREP; rep.cols = wv->cols;
        CK(h->dalloc(one * VAE_VREP, &rep.p));
        for (int i = 0; i < VAE_VREP; ++i)
            DSIM_HIP_CHECK(hipMemcpyAsync((char*)rep.p + i * one, wv->p, one, hipMemcpyDeviceToDevice, s));
        h->pk["encoder.mid_block.attentions.0.to_v.weight_rep"] = rep;
    }
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    h->raw.clear();
    h->finalized = true;
    Arena ar;
    VWalk w{h, &ar, s, 1, false};
    const int st = w.go(nullptr, 8 << (h->cfg.n_levels - 1), nullptr);
    if (st != DSIM_OK) { h->finalized = false; return st; }
    return DSIM_OK;
}

// dry walk of an encode: peak arena bytes
static int vae_plan(dsim_vae* h, int n_images, int image_size, size_t* peak) {
    Arena ar;
    VWalk w{h, &ar, nullptr, n_images, false};
    CK(w.go(nullptr, image_size, nullptr));
    if (w.max_tensor >= 0x7fffffffull) return DSIM_ERR_INVALID;      // a >= 2 GiB activation: the batch does not fit one call (32-bit tensor offsets)
    *peak = ar.peak;
    return DSIM_OK;
}

size_t dsim_vae_workspace_bytes(const dsim_vae* hc, int n_images, int image_size) {
    dsim_vae* h = const_cast<dsim_vae*>(hc);
    if (!h || !h->finalized || n_images < 1 || image_size < (1 << (h->cfg.n_levels - 1))) return 0;
    size_t peak;
    if (vae_plan(h, n_images, image_size, &peak) != DSIM_OK) return 0;
    return peak + 256;
}

int dsim_vae_encode(dsim_vae* h, const float* images, int n_images, int image_size, float* moments, void* workspace,
                    size_t workspace_bytes, void* stream) {
    if (!h || !images || !moments || !workspace || n_images < 1) return DSIM_ERR_INVALID;
    if (!h->finalized) return DSIM_ERR_STATE;
    if (image_size % (1 << (h->cfg.n_levels - 1))) return DSIM_ERR_INVALID;
    return run_in_workspace(
        workspace, workspace_bytes, [&](size_t* peak) { return vae_plan(h, n_images, image_size, peak); },
        [&](Arena& ar) {
            VWalk w{h, &ar, (hipStream_t)stream, n_images, true};
            return w.go(images, image_size, moments);
        });
}

int dsim_vae_profile(dsim_vae* h, int enable) { return prof_enable(h, enable); }
int dsim_vae_profile_count(const dsim_vae* h) { return prof_count(h); }
int dsim_vae_profile_get(dsim_vae* h, int i, char* name, int name_cap, double* flops, double* bytes, double* ms) {
    return prof_get(h, i, name, name_cap, flops, bytes, ms);
}

int dsim_image_preprocess(const unsigned char* pixels_hwc, float* out, int n, int H, int W, int to_half, void* stream) {
    return image_preprocess(pixels_hwc, out, n, H, W, to_half != 0, (hipStream_t)stream);
}

int dsim_latent_sample(const float* moments, const float* eps, float* out, int n_out, int first, int stride, int C, int hw,
                       int eps_n, float scaling_factor, int round_fp16, void* stream) {
    return latent_sample(moments, eps, out, n_out, first, stride, C, hw, eps_n, scaling_factor, round_fp16 != 0, (hipStream_t)stream);
}

}  // extern "C"
