// ViT executor (normalised pixels -> tapped self-attention q/k/v) and its C ABI: the backbone of the reference's clip_cross and
// dino_cross metrics.
//
// Replaces, for the reference's metrics/clip_i.py:113-159 (CLIPScore.clip_cross_score) and metrics/dino.py:120-161
// (Dinov2Score.dino_cross_score), the forward of HF CLIPVisionModel / Dinov2Model up to the hooked layer and the hook itself
// (metrics/hooks.py:3-32), which re-projects the hooked module's input with the layer's own q / k / v Linear layers.
// Graph (pre-LN transformer; DINOv2: LayerScale on, erf-GELU, patch bias; CLIP: pre_layrnorm, quick-GELU, no patch bias):
//     tokens = [cls ; patch_conv(pixels), row-major] + pos                 (patch rows -> GEMM -> token assembly; pos arrives already interpolated)
//     h_0 = pre_norm ? LN(tokens) : tokens
//     h'  = h  + ls1 * proj(SDPA(qkv(LN1(h))))
//     h'' = h' + ls2 * fc2(act(fc1(LN2(h'))))
// Tap at block L: q, k, v = the three row blocks of the fused qkv Linear applied to LN1(h_L) (tap_input 0: DINOv2, whose hook sits on
// attention.attention) or to h_L itself (tap_input 1: CLIP, whose hook sits on the encoder layer -- the reference's quirk, kept).
// Kernels: the patch rows, the class-token / position assembly and the two activations (here); LayerNorm (norm.hip), the MFMA GEMM with bias /
// LayerScale-gate + residual epilogues (gemm.hip: LayerScale is its per-column gate with no second half), attention at D = 64
// (attention.hip).  Weights under one neutral naming (include/diffsim_amd.h); the Python side maps the HF keys onto it.
#include <string>
#include <vector>

#include "common.h"
#include "store.h"

using namespace dsim;

struct dsim_vit : WeightStore {
    dsim_vit_cfg cfg;
    void* patch_w = nullptr;    // [C][Kp] in the compute dtype: the patch conv as a Linear, K = 3 p p zero-padded (finalize)
    int Kp = 0;
};

namespace {

// The patch conv as a Linear: K = 3 p p is 588 (DINOv2 /14), 768 (/16), 3072 (CLIP /32) or 192 (the test configs), zero-padded to a
// multiple of 64 (Kp: the GEMM's K tile) on both operands.  vit_patches_kernel writes the patch rows, the MFMA GEMM multiplies them by
// the padded weight (+ bias), vit_tokens_kernel puts the class token in front and adds the positions.  (A direct f32 kernel ran
// CLIP-B/32's embedding of 512 images in 18.5 ms, 72 % of the forward to layer 11; this form takes the GEMM's time.)
constexpr int V8 = 8;       // elements per thread of the three element-wise kernels (C, Kp and the MLP width are multiples of 8)
template <typename T> struct Vec8 { typedef T type __attribute__((ext_vector_type(V8))); };

// pixels f32 [n][3][S][S] -> A [n * T][Kp] in the compute dtype, row (img, tok), column k = (c, py, px) as the conv weight's rows are
// laid out, zeros for k >= K; groups = n * T * Kp / 8
template <typename T>
__global__ __launch_bounds__(256) void vit_patches_kernel(const float* __restrict__ pix, T* __restrict__ A, int S, int p, int Kp, size_t groups) {
    const int K = 3 * p * p, g = S / p, Ttok = g * g, kg = Kp / V8;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < groups; i += (size_t)gridDim.x * 256) {
        const size_t row = i / kg;
        const int k0 = (int)(i - row * kg) * V8;
        const int img = (int)(row / Ttok), tok = (int)(row - (size_t)img * Ttok), ty = tok / g, tx = tok - ty * g;
        typename Vec8<T>::type v;
#pragma unroll
        for (int e = 0; e < V8; ++e) {
            const int k = k0 + e;
            float x = 0.f;
            if (k < K) {
                const int c = k / (p * p), r = k - c * p * p, py = r / p, px = r - py * p;
                x = pix[(((size_t)img * 3 + c) * S + ty * p + py) * S + tx * p + px];
            }
            v[e] = (T)x;
        }
        *(typename Vec8<T>::type*)(A + i * V8) = v;
    }
}

// conv weight f32 [D][K] -> [D][Kp] in the compute dtype, zero-padded (once, at finalize)
template <typename T>
__global__ __launch_bounds__(256) void vit_pack_patch_w_kernel(const float* __restrict__ w, T* __restrict__ out, int K, int Kp, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t d = i / Kp;
    const int k = (int)(i - d * Kp);
    out[i] = k < K ? (T)w[d * K + k] : (T)0.f;
}

// tokens [n][N][D] = [cls ; emb rows of the image] + pos, emb [n * T][D] the GEMM's output; groups = n * N * D / 8
template <typename T>
__global__ __launch_bounds__(256) void vit_tokens_kernel(const T* __restrict__ emb, const float* __restrict__ cls, const float* __restrict__ pos,
                                                         T* __restrict__ out, int Ttok, int D, size_t groups) {
    const int N = Ttok + 1, dg = D / V8;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < groups; i += (size_t)gridDim.x * 256) {
        const size_t row = i / dg;
        const int d0 = (int)(i - row * dg) * V8;
        const size_t img = row / N;
        const int t = (int)(row - img * N);
        typename Vec8<T>::type v;
        if (t > 0) v = *(const typename Vec8<T>::type*)(emb + (img * Ttok + t - 1) * D + d0);
#pragma unroll
        for (int e = 0; e < V8; ++e) v[e] = (T)((t > 0 ? (float)v[e] : cls[d0 + e]) + pos[(size_t)t * D + d0 + e]);
        *(typename Vec8<T>::type*)(out + i * V8) = v;
    }
}

// the MLP activation, in place on n elements of the compute dtype (n % 8 == 0), evaluated in f32: erf-GELU (F.gelu's default:
// DINOv2) or quick-GELU x sigmoid(1.702 x) (CLIP)
__device__ __forceinline__ float vit_act(float x, int act) {
    if (act == DSIM_VIT_ACT_QUICK_GELU) return x / (1.0f + expf(-1.702f * x));
    return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f));
}
template <typename T>
__global__ __launch_bounds__(256) void vit_act_kernel(T* __restrict__ x, size_t groups, int act) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < groups; i += (size_t)gridDim.x * 256) {
        typename Vec8<T>::type v = *(typename Vec8<T>::type*)(x + i * V8);
#pragma unroll
        for (int e = 0; e < V8; ++e) v[e] = (T)vit_act((float)v[e], act);
        *(typename Vec8<T>::type*)(x + i * V8) = v;
    }
}

inline unsigned ew_blocks(size_t groups) {
    const size_t b = (groups + 255) / 256;
    return (unsigned)(b < 65536 ? (b ? b : 1) : 65536);
}

int vit_patches(const float* pix, void* A, int dtype, int n_img, int S, int p, int Kp, hipStream_t s) {
    const size_t groups = (size_t)n_img * (S / p) * (S / p) * Kp / V8;
    return by_dtype(dtype, [&](auto e) {
        typedef typename decltype(e)::type T_;
        hipLaunchKernelGGL(vit_patches_kernel<T_>, dim3(ew_blocks(groups)), dim3(256), 0, s, pix, (T_*)A, S, p, Kp, groups);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

int vit_pack_patch_w(const float* w, void* out, int dtype, int D, int K, int Kp, hipStream_t s) {
    const size_t total = (size_t)D * Kp;
    return by_dtype(dtype, [&](auto e) {
        typedef typename decltype(e)::type T_;
        hipLaunchKernelGGL(vit_pack_patch_w_kernel<T_>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, (T_*)out, K, Kp, total);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

int vit_tokens(const void* emb, const float* cls, const float* pos, void* out, int dtype, int n_img, int Ttok, int D, hipStream_t s) {
    const size_t groups = (size_t)n_img * (Ttok + 1) * D / V8;
    return by_dtype(dtype, [&](auto e) {
        typedef typename decltype(e)::type T_;
        hipLaunchKernelGGL(vit_tokens_kernel<T_>, dim3(ew_blocks(groups)), dim3(256), 0, s, (const T_*)emb, cls, pos, (T_*)out, Ttok, D, groups);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

int vit_activation(void* x, size_t n, int act, int dtype, hipStream_t s) {
    return by_dtype(dtype, [&](auto e) {
        typedef typename decltype(e)::type T_;
        hipLaunchKernelGGL(vit_act_kernel<T_>, dim3(ew_blocks(n / V8)), dim3(256), 0, s, (T_*)x, n / V8, act);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

// one tap of a walk: the block and the tensors that receive its q, k, v
struct VTap {
    int layer;
    void *q = nullptr, *k = nullptr, *v = nullptr;
};

struct ViTWalk : WalkBase<dsim_vit> {
    const int n;            // images
    std::vector<VTap> taps; // captured on the way; the walk ends at the deepest
    bool tapped = false;
    ViTWalk(dsim_vit* h, Arena* ar, hipStream_t s, int n, bool run) : WalkBase(h, ar, s, run), n(n) {}

    // out = a w^T + bias, or residual + gate * (a w^T + bias) (gate: a LayerScale vector or null)
    int linear(const void* a, int K, const void* w, const float* bias, void* out, int M, int N, const float* gate, const void* residual) {
        GemmArgs g = linear_args(a, K, w, bias, residual, out, M, N);
        if (gate) { g.gate = gate; g.rows_per_batch = M; }
        return gemm(g);
    }
    int ln(const void* x, const Packed* gw, const Packed* gb, void* out, int M, int C) {
        return launch([&] { return rec(std::string("layernorm_") + dtn() + "|M" + std::to_string(M) + " C" + std::to_string(C), 0.0,
                                       2.0 * M * (double)C * es()); },
                      [&] { return launch_layernorm(x, (const float*)gw->p, (const float*)gb->p, out, M, C, h->cfg.ln_eps, h->dt, s); });
    }

    int go(const float* pix) {
        const dsim_vit_cfg& c = h->cfg;
        const int C = c.hidden_size, p = c.patch_size, S = c.image_size, g = S / p, N = g * g + 1, H = c.num_heads, F = c.mlp_dim;
        const int M = n * N;
        const int Tt = g * g, Kp = h->Kp;
        const size_t widest = (size_t)(F > 3 * C ? F : 3 * C);
        if ((size_t)M * (widest > (size_t)Kp ? widest : (size_t)Kp) * es() >= 0x7fffffffull) return DSIM_ERR_INVALID;     // 32-bit tensor offsets
        WGET(pw, "x_embedder.proj.weight"); WGET(cls, "cls_token"); WGET(pos, "pos_embed");
        const Packed* pb = nullptr;
        if (c.patch_bias) { WGET(pb_, "x_embedder.proj.bias"); pb = pb_; }
        if (pos->rows != N || pos->cols != C || pw->rows != C || pw->cols != 3 * p * p || !h->patch_w) return DSIM_ERR_INVALID;
        void* x = alloc_act((size_t)M * C);
        void* nb = alloc_act((size_t)M * C);
        void* big = alloc_act((size_t)M * widest);
        void* ab = alloc_act((size_t)M * C);
        {
            // the embedding: patch rows (an arena temporary) -> GEMM into nb -> tokens in x
            const size_t mk = ar->mark();
            void* A = alloc_act((size_t)n * Tt * Kp);
            CK(launch([&] { return rec(std::string("vit_patches_") + dtn() + "|n" + std::to_string(n) + " T" + std::to_string(Tt) + " K" +
                                           std::to_string(Kp), 0.0, 4.0 * n * 3.0 * S * S + (double)n * Tt * Kp * es()); },
                      [&] { return vit_patches(pix, A, h->dt, n, S, p, Kp, s); }));
            CK(linear(A, Kp, h->patch_w, pb ? (const float*)pb->p : nullptr, nb, n * Tt, C, nullptr, nullptr));
            CK(launch([&] { return rec(std::string("vit_tokens_") + dtn() + "|n" + std::to_string(n) + " N" + std::to_string(N) + " C" +
                                           std::to_string(C), 0.0, ((double)n * Tt + M) * C * es()); },
                      [&] { return vit_tokens(nb, (const float*)cls->p, (const float*)pos->p, x, h->dt, n, Tt, C, s); }));
            ar->release(mk);
        }
        if (c.pre_norm) {
            WGET(gw, "pre_norm.weight"); WGET(gb, "pre_norm.bias");
            CK(ln(x, gw, gb, nb, M, C));
            void* t = x; x = nb; nb = t;
        }
        int last = -1;
        for (const VTap& t : taps) last = t.layer > last ? t.layer : last;
        for (int blk = 0; blk <= last; ++blk) {
            const std::string b = "blocks." + std::to_string(blk) + ".";
            WGET(n1w, b + "norm1.weight"); WGET(n1b, b + "norm1.bias");
            WGET(qw, b + "attn.qkv.weight"); WGET(qb, b + "attn.qkv.bias");
            if (blk < last || !c.tap_input) CK(ln(x, n1w, n1b, nb, M, C));
            for (const VTap& t : taps) {
                if (t.layer != blk) continue;
                // the hook's input (norm1's output, or the block's own input): q/k/v = row blocks of the fused qkv Linear
                const void* src = c.tap_input ? x : nb;
                for (int j = 0; j < 3; ++j) {
                    void* dst = j == 0 ? t.q : (j == 1 ? t.k : t.v);
                    CK(linear(src, C, (char*)qw->p + (size_t)j * C * C * es(), (const float*)qb->p + (size_t)j * C, dst, M, C, nullptr, nullptr));
                }
            }
            if (blk == last) {
                tapped = true;
                return DSIM_OK;
            }
            WGET(ow, b + "attn.proj.weight"); WGET(ob, b + "attn.proj.bias");
            WGET(n2w, b + "norm2.weight"); WGET(n2b, b + "norm2.bias");
            WGET(f1w, b + "mlp.fc1.weight"); WGET(f1b, b + "mlp.fc1.bias");
            WGET(f2w, b + "mlp.fc2.weight"); WGET(f2b, b + "mlp.fc2.bias");
            const float *ls1 = nullptr, *ls2 = nullptr;
            if (c.layer_scale) {
                WGET(l1, b + "ls1"); WGET(l2, b + "ls2");
                ls1 = (const float*)l1->p; ls2 = (const float*)l2->p;
            }
            CK(linear(nb, C, qw->p, (const float*)qb->p, big, M, 3 * C, nullptr, nullptr));
            AttnArgs a;
            a.q = big; a.ldq = 3 * C;
            a.k = (char*)big + (size_t)C * es(); a.v = (char*)big + (size_t)2 * C * es(); a.ldk = 3 * C;
            a.out = ab; a.ldo = C; a.B = n; a.Bkv = n; a.H = H; a.Nq = N; a.Nk = N; a.D = C / H;
            CK(launch([&] { return attn_rec(a); }, [&] { return launch_attention(a, h->dt, s); }));
            CK(linear(ab, C, ow->p, (const float*)ob->p, x, M, C, ls1, x));
            CK(ln(x, n2w, n2b, nb, M, C));
            CK(linear(nb, C, f1w->p, (const float*)f1b->p, big, M, F, nullptr, nullptr));
            CK(launch([&] { return rec(std::string(c.act == DSIM_VIT_ACT_QUICK_GELU ? "act_quick_gelu_" : "act_gelu_") + dtn() + "|M" +
                                           std::to_string(M) + " F" + std::to_string(F), 0.0, 2.0 * M * (double)F * es()); },
                      [&] { return vit_activation(big, (size_t)M * F, c.act, h->dt, s); }));
            CK(linear(big, F, f2w->p, (const float*)f2b->p, x, M, C, ls2, x));
        }
        return DSIM_ERR_INVALID;
    }
};

// dry walk to the deepest of `taps`: peak arena bytes
int vit_plan(dsim_vit* h, int n_images, const std::vector<VTap>& taps, size_t* peak) {
    Arena ar;
    ViTWalk w{h, &ar, nullptr, n_images, false};
    w.taps = taps;
    CK(w.go(nullptr));
    *peak = ar.peak;
    return DSIM_OK;
}

// the layers of one sweep, checked: each in [0, depth), no two alike
int vit_check_taps(const dsim_vit* h, int n_taps, const int* layers, std::vector<VTap>* out) {
    if (n_taps < 1 || !layers) return DSIM_ERR_INVALID;
    out->clear();
    for (int i = 0; i < n_taps; ++i) {
        if (layers[i] < 0 || layers[i] >= h->cfg.depth) return DSIM_ERR_INVALID;
        for (int j = 0; j < i; ++j)
            if (layers[j] == layers[i]) return DSIM_ERR_INVALID;
        out->push_back(VTap{layers[i]});
    }
    return DSIM_OK;
}

// one walk to the deepest of `taps` (their outputs set), every check before the first launch
int vit_run(dsim_vit* h, const float* pixels, int n_images, const std::vector<VTap>& taps, void* workspace, size_t workspace_bytes,
            void* stream) {
    bool tapped = false;
    CK(run_in_workspace(
        workspace, workspace_bytes, [&](size_t* peak) { return vit_plan(h, n_images, taps, peak); },
        [&](Arena& ar) {
            ViTWalk w{h, &ar, (hipStream_t)stream, n_images, true};
            w.taps = taps;
            const int st = w.go(pixels);
            tapped = w.tapped;
            return st;
        }));
    return tapped ? DSIM_OK : DSIM_ERR_WORKSPACE;
}

}  // namespace

extern "C" {

int dsim_vit_create(const dsim_vit_cfg* cfg, dsim_vit** out) {
    if (!cfg || !out) return DSIM_ERR_INVALID;
    if (cfg->image_size < 1 || cfg->patch_size < 1 || cfg->hidden_size < 1 || cfg->depth < 1 || cfg->num_heads < 1 || cfg->mlp_dim < 1)
        return DSIM_ERR_INVALID;
    if (cfg->tap_layer < 0 || cfg->tap_layer >= cfg->depth || cfg->hidden_size % cfg->num_heads || cfg->image_size % cfg->patch_size)
        return DSIM_ERR_INVALID;
    if (cfg->act != DSIM_VIT_ACT_GELU && cfg->act != DSIM_VIT_ACT_QUICK_GELU) return DSIM_ERR_INVALID;
    if ((cfg->tap_input != 0 && cfg->tap_input != 1) || !(cfg->ln_eps > 0.f)) return DSIM_ERR_INVALID;
    if (cfg->hidden_size % 8 || cfg->mlp_dim % 8) return DSIM_ERR_INVALID;      // the element-wise kernels work on groups of 8
    return handle_create(cfg, out);
}

void dsim_vit_destroy(dsim_vit* h) { delete h; }

int dsim_vit_load_weight(dsim_vit* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim) {
    return handle_load(h, key, dev_ptr, dtype, shape, ndim);
}

int dsim_vit_finalize(dsim_vit* h, void* stream) {
    if (!h) return DSIM_ERR_INVALID;
    if (h->finalized) return DSIM_ERR_STATE;
    hipStream_t s = (hipStream_t)stream;
    CK(pack_all(h, s));
    {
        // the patch conv as a Linear: [C][3 p p] f32 (pack_all's flat copy) -> [C][Kp] in the compute dtype, zero-padded
        const int C = h->cfg.hidden_size, K = 3 * h->cfg.patch_size * h->cfg.patch_size;
        const Packed* pw = h->find("x_embedder.proj.weight");
        if (!pw) return DSIM_ERR_MISSING_WEIGHT;
        if (pw->rows != C || pw->cols != K) return DSIM_ERR_INVALID;
        h->Kp = (K + 63) / 64 * 64;
        CK(h->dalloc((size_t)C * h->Kp * dtype_size(h->dt), &h->patch_w));
        CK(vit_pack_patch_w((const float*)pw->p, h->patch_w, h->dt, C, K, h->Kp, s));
    }
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    h->raw.clear();
    h->finalized = true;
    size_t peak;
    const int st = vit_plan(h, 1, {VTap{h->cfg.tap_layer}}, &peak);
    if (st != DSIM_OK) { h->finalized = false; return st; }
    return DSIM_OK;
}

int dsim_vit_set_tap(dsim_vit* h, int tap_layer) {
    if (!h || tap_layer < 0 || tap_layer >= h->cfg.depth) return DSIM_ERR_INVALID;
    if (!h->finalized) return DSIM_ERR_STATE;
    const int old = h->cfg.tap_layer;
    if (tap_layer == old) return DSIM_OK;
    h->cfg.tap_layer = tap_layer;
    size_t peak;                                // every parameter up to the new tap must have been loaded: dry walk
    const int st = vit_plan(h, 1, {VTap{tap_layer}}, &peak);
    if (st != DSIM_OK) { h->cfg.tap_layer = old; return st; }
    return DSIM_OK;
}

int dsim_vit_profile(dsim_vit* h, int enable) { return prof_enable(h, enable); }
int dsim_vit_profile_count(const dsim_vit* h) { return prof_count(h); }
int dsim_vit_profile_get(dsim_vit* h, int i, char* name, int name_cap, double* flops, double* bytes, double* ms) {
    return prof_get(h, i, name, name_cap, flops, bytes, ms);
}

size_t dsim_vit_workspace_bytes(const dsim_vit* hc, int n_images) {
    dsim_vit* h = const_cast<dsim_vit*>(hc);
    if (!h || !h->finalized || n_images < 1) return 0;
    size_t peak;
    if (vit_plan(h, n_images, {VTap{h->cfg.tap_layer}}, &peak) != DSIM_OK) return 0;
    return peak + 256;
}

size_t dsim_vit_taps_workspace_bytes(const dsim_vit* hc, int n_images, int n_taps, const int* layers) {
    dsim_vit* h = const_cast<dsim_vit*>(hc);
    if (!h || !h->finalized || n_images < 1) return 0;
    std::vector<VTap> taps;
    size_t peak;
    if (vit_check_taps(h, n_taps, layers, &taps) != DSIM_OK || vit_plan(h, n_images, taps, &peak) != DSIM_OK) return 0;
    return peak + 256;
}

int dsim_vit_qkv(dsim_vit* h, const float* pixels, int n_images, void* q, void* k, void* v, void* workspace, size_t workspace_bytes,
                 void* stream) {
    if (!h || !pixels || !q || !k || !v || !workspace || n_images < 1) return DSIM_ERR_INVALID;
    if (!h->finalized) return DSIM_ERR_STATE;
    VTap t{h->cfg.tap_layer};
    t.q = q; t.k = k; t.v = v;
    return vit_run(h, pixels, n_images, {t}, workspace, workspace_bytes, stream);
}

int dsim_vit_qkv_taps(dsim_vit* h, const float* pixels, int n_images, int n_taps, const int* layers, void* const* q, void* const* k,
                      void* const* v, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !pixels || !q || !k || !v || !workspace || n_images < 1) return DSIM_ERR_INVALID;
    if (!h->finalized) return DSIM_ERR_STATE;
    std::vector<VTap> taps;
    CK(vit_check_taps(h, n_taps, layers, &taps));
    for (int i = 0; i < n_taps; ++i) {
        if (!q[i] || !k[i] || !v[i]) return DSIM_ERR_INVALID;
        taps[i].q = q[i]; taps[i].k = k[i]; taps[i].v = v[i];
    }
    return vit_run(h, pixels, n_images, taps, workspace, workspace_bytes, stream);
}

}  // extern "C"
