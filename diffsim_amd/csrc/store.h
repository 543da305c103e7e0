// Shared host-side plumbing of the executors (U-Net, VAE, DiT): borrowed raw parameters, packed device copies, the
// caller-provided workspace arena, the per-launch profiling record, the handle life cycle behind each dsim_<executor>_create /
// destroy / load_weight / profile* group (handle_create ... prof_get) and the base of the three graph walks (WalkBase).
// WalkBase holds what every step of a walk is made of: launch() -- the one bracket around a kernel launch (nothing on a dry walk, a
// profile record around it on a profiled one, the launch's status) --, the records of the launch kinds the walks share (gemm,
// attention, GroupNorm), and the two GemmArgs builders (linear_args, conv3_args) each walk's linear / conv3 starts from.  An
// activation (Act) carries its own batch count: no step reads how many batch elements it works on from anywhere else.
#pragma once
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "common.h"

namespace dsim {

struct RawW { const void* p; int dtype; std::vector<int64_t> shape; };

struct Packed { void* p = nullptr; size_t bytes = 0; int rows = 0, cols = 0; };

struct Arena {
    char* base = nullptr;
    size_t cap = 0, off = 0, peak = 0;
    bool dry = true;
    bool overflow = false;
    void* alloc(size_t bytes) {
        const size_t a = (off + 255) & ~(size_t)255;
        off = a + bytes;
        if (off > peak) peak = off;
        if (!dry && off > cap) { overflow = true; return nullptr; }
        return dry ? (void*)(uintptr_t)(a + 256) : (void*)(base + a);   // non-null dummy when planning
    }
    size_t mark() const { return off; }
    void release(size_t m) { off = m; }
};

// a token-major activation [B][H * W][C] in the compute dtype
struct Act {
    void* p = nullptr;
    int C = 0, H = 0, W = 0, B = 0;
    int rows() const { return B * H * W; }
};

// per-launch record of a profiled forward (dsim_*_profile_*): kernel family, algorithmic work
// and the HIP-event bracket on the launch stream
struct ProfRec {
    std::string name;
    double flops = 0, bytes = 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0.f;
};

#define CK(expr)                         \
    do {                                 \
        int _s = (expr);                 \
        if (_s != DSIM_OK) return _s;    \
    } while (0)

static inline bool ends_with(const std::string& s, const char* suf) {
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

// parameters of one model: raw (borrowed until finalize) and packed (owned device buffers)
struct WeightStore {
    int dt = DSIM_BF16;
    bool finalized = false;
    std::map<std::string, RawW> raw;
    std::map<std::string, Packed> pk;
    std::vector<void*> owned;
    void* zero_page = nullptr;
    std::string err_key;
    bool profiling = false;
    std::vector<ProfRec> prof;

    int dalloc(size_t bytes, void** out) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return DSIM_ERR_HIP;
        owned.push_back(p);
        *out = p;
        return DSIM_OK;
    }
    const Packed* find(const std::string& k) {
        auto it = pk.find(k);
        if (it == pk.end()) { err_key = k; return nullptr; }
        return &it->second;
    }
    // (a handle destroyed with profile records pending releases their events too)
    ~WeightStore() {
        clear_profile();
        for (void* p : owned) (void)hipFree(p);
    }
    int add_raw(const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim) {
        if (!key || !dev_ptr || !shape || ndim < 1 || ndim > 4) return DSIM_ERR_INVALID;
        if (dtype != DSIM_F32 && dtype != DSIM_BF16 && dtype != DSIM_F16) return DSIM_ERR_INVALID;
        if (finalized) return DSIM_ERR_STATE;
        RawW w;
        w.p = dev_ptr; w.dtype = dtype; w.shape.assign(shape, shape + ndim);
        raw[key] = w;
        return DSIM_OK;
    }
    void clear_profile() {
        for (auto& r : prof) {
            if (r.e0) (void)hipEventDestroy(r.e0);
            if (r.e1) (void)hipEventDestroy(r.e1);
        }
        prof.clear();
    }
};

// profile family of a GEMM launch = the kernel symbol launch_gemm will pick for it (one family per symbol), composed from gemm_plan()'s
// answer alone, + its algorithmic work.  Epilogue suffixes: _geglu | _res | _act (tanh-GELU only) | _dit (the gated DiT epilogues,
// residual or not), + _gn for the statistics epilogue kinds.  (A problem launch_gemm refuses: "gemm_<dtype>_refused".)
static inline std::string gemm_family(const GemmArgs& g, int dt, double* flops, double* bytes) {
    GemmLaunchRec p;
    const bool ok = gemm_plan(g, dt, &p) == DSIM_OK;
    const char* dtn = dtype_name(dt);
    const double e = (double)dtype_size(dt);
    const double outc = g.epi == EPI_GEGLU ? g.N / 2 : g.N;
    *flops = 2.0 * g.M * (double)g.N * g.K;
    *bytes = e * ((double)g.M * (g.mode == GEMM_CONV3 ? g.C0 : g.K) + (double)g.N * g.K * (g.wb_rows ? g.M / g.wb_rows : 1) +
                  (double)g.M * outc * (g.residual ? 2 : 1));
    static const char* const kind[] = {"_linear", "_conv3", "_conv3p"};
    static const char* const epi[] = {"", "_res", "_dit", "_act", "_gn", "_res_gn"};      // by EK_*
    const std::string size = "|M" + std::to_string(g.M) + " N" + std::to_string(g.N) + " K" + std::to_string(g.K);
    if (!ok) return std::string("gemm_") + dtn + "_refused" + size;
    return std::string(p.small ? "gemm_small_" : "gemm_") + dtn + "_" + std::to_string(p.bm) + "x" + std::to_string(p.bn) + kind[p.mode] +
           (p.geglu ? "_geglu" : epi[p.ek]) + size;
}

// HIP-event bracket of one launch of a profiled forward (WalkBase::launch); r: name and work of the launch
static inline void prof_begin(WeightStore* h, hipStream_t s, ProfRec r) {
    (void)hipEventCreate(&r.e0);
    (void)hipEventCreate(&r.e1);
    (void)hipEventRecord(r.e0, s);
    h->prof.push_back(r);
}
static inline void prof_end(WeightStore* h, hipStream_t s) { (void)hipEventRecord(h->prof.back().e1, s); }
static inline int prof_get(WeightStore* h, int i, char* name, int name_cap, double* flops, double* bytes, double* ms) {
    if (!h || i < 0 || i >= (int)h->prof.size() || !name || name_cap < 2 || !flops || !bytes || !ms) return DSIM_ERR_INVALID;
    ProfRec& r = h->prof[i];
    if (r.e0 && r.e1) {
        DSIM_HIP_CHECK(hipEventSynchronize(r.e1));
        DSIM_HIP_CHECK(hipEventElapsedTime(&r.ms, r.e0, r.e1));
    }
    strncpy(name, r.name.c_str(), (size_t)name_cap - 1);
    name[name_cap - 1] = 0;
    *flops = r.flops; *bytes = r.bytes; *ms = (double)r.ms;
    return DSIM_OK;
}

// ---- handle life cycle: what dsim_unet_* / dsim_vae_* / dsim_dit_* forward to ------------------------------------------------
// create, after the executor's own validation of cfg: H = the handle (a WeightStore with a `cfg` member)
template <class H, class Cfg>
static inline int handle_create(const Cfg* cfg, H** out) {
    if (cfg->compute_dtype != DSIM_F32 && cfg->compute_dtype != DSIM_BF16 && cfg->compute_dtype != DSIM_F16) return DSIM_ERR_INVALID;
    if (dsim_device_count() < 1) return DSIM_ERR_NO_DEVICE;
    H* h = new H();
    h->cfg = *cfg;
    h->dt = cfg->compute_dtype;
    if (h->dalloc(256, &h->zero_page) != DSIM_OK || hipMemset(h->zero_page, 0, 256) != hipSuccess) {
        delete h;
        return DSIM_ERR_HIP;
    }
    *out = h;
    return DSIM_OK;
}
static inline int handle_load(WeightStore* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim) {
    return h ? h->add_raw(key, dev_ptr, dtype, shape, ndim) : DSIM_ERR_INVALID;
}
static inline int prof_enable(WeightStore* h, int enable) {
    if (!h) return DSIM_ERR_INVALID;
    h->clear_profile();
    h->profiling = enable != 0;
    return DSIM_OK;
}
static inline int prof_count(const WeightStore* h) { return h ? (int)h->prof.size() : 0; }

// ---- one call on a caller's workspace ------------------------------------------------------------------------------------------
// a caller's workspace starts at its first 256-byte boundary: moves `ws` there and takes the bytes before it off `bytes`; false when
// the buffer does not reach it
static inline bool align_workspace(void*& ws, size_t& bytes) {
    const uintptr_t b0 = ((uintptr_t)ws + 255) & ~(uintptr_t)255;
    const size_t lost = b0 - (uintptr_t)ws;
    if (bytes < lost) return false;
    ws = (void*)b0;
    bytes -= lost;
    return true;
}

// plan(&peak): the dry walk; walk(arena): the same walk launching.  Refuses up front, before the first launch, instead of failing
// mid-graph; DSIM_OK = walked without leaving the arena.
template <class Plan, class Run>
static inline int run_in_workspace(void* ws, size_t bytes, Plan plan, Run walk) {
    if (!align_workspace(ws, bytes)) return DSIM_ERR_WORKSPACE;
    size_t peak = 0;
    CK(plan(&peak));
    if (peak > bytes) return DSIM_ERR_WORKSPACE;
    Arena ar;
    ar.dry = false;
    ar.base = (char*)ws;
    ar.cap = bytes;
    CK(walk(ar));
    return ar.overflow ? DSIM_ERR_WORKSPACE : DSIM_OK;
}

// ---- base of the executors' walks (Walk / VWalk / DWalk): one struct runs dry to plan the workspace and for real to launch ------
#define WGET(var, key)                                   \
    const Packed* var = h->find(key);                    \
    if (!var) return DSIM_ERR_MISSING_WEIGHT;

namespace {      // internal linkage, as the rest of this header and the walks that derive from it

template <class H>
struct WalkBase {
    H* h;
    Arena* ar;
    hipStream_t s;
    bool run;               // false: plan only
    size_t max_tensor = 0;  // largest single activation (bytes): the kernels address tensors with 32-bit offsets
    WalkBase(H* h_, Arena* ar_, hipStream_t s_, bool run_) : h(h_), ar(ar_), s(s_), run(run_) {}

    size_t es() const { return dtype_size(h->dt); }
    void* alloc_act(size_t elems) {
        if (elems * es() > max_tensor) max_tensor = elems * es();
        return ar->alloc(elems * es());
    }
    Act act(int B, int Hh, int Ww, int C) { return Act{alloc_act((size_t)B * Hh * Ww * C), C, Hh, Ww, B}; }      // a new activation on the arena
    const char* dtn() const { return dtype_name(h->dt); }

    // ---- the launch bracket: every kernel launch of a walk goes through one of these two ------------------------------------------
    // rec() -> ProfRec{name, flops, bytes}, called on a profiled forward only (an unprofiled one builds no string); go() launches and
    // returns the status.  Nothing on a dry walk.
    template <class Rec, class Go>
    int launch(Rec&& rec, Go&& go) {
        if (!run) return DSIM_OK;
        if (!h->profiling) return go();
        prof_begin(h, s, rec());
        const int st = go();
        prof_end(h, s);
        return st;
    }
    // a launch that has no profile record
    template <class Go>
    int launch(Go&& go) { return run ? go() : DSIM_OK; }

    static ProfRec rec(std::string name, double flops, double bytes) {
        ProfRec r;
        r.name = std::move(name); r.flops = flops; r.bytes = bytes;
        return r;
    }
    // the record of an attention launch; fp8: the e4m3 kernel (attention_fp8.hip), its own family
    // (key sequences >= 2048 run the fixed-reference instantiation attn_kernel<T, D, true>: its own family)
    ProfRec attn_rec(const AttnArgs& a, bool fp8 = false) const {
        return rec((fp8 ? std::string("attention_fp8_d") + std::to_string(a.D)
                        : std::string("attention_") + dtn() + "_d" + std::to_string(a.D) + attention_kernel_kind(a, h->dt)) +
                       "|B" + std::to_string(a.B) + " H" + std::to_string(a.H) + " Nq" + std::to_string(a.Nq) + " Nk" + std::to_string(a.Nk),
                   4.0 * a.B * a.H * (double)a.Nq * a.Nk * a.D, (double)es() * a.B * a.H * a.D * (2.0 * a.Nq + 2.0 * a.Nk));
    }
    // the record of a GroupNorm launch over B x HW x (C0 + C1); pre: statistics from the producing conv's epilogue (apply pass only)
    ProfRec gn_rec(int B, int HW, int C0, int C1, int groups, bool pre = false) const {
        const double n = (double)B * HW * (C0 + C1);
        return rec(std::string(pre ? "groupnorm_pre_" : "groupnorm_") + dtn() + "|B" + std::to_string(B) + " HW" + std::to_string(HW) + " C" +
                       std::to_string(C0 + C1), 0.0,
                   (pre ? 2.0 : (double)groupnorm_passes(C0, C1, HW, groups, h->dt)) * n * es());
    }

    int gemm(GemmArgs& g) {
        g.zero_page = h->zero_page;
        return launch(
            [&] {
                ProfRec r;
                r.name = gemm_family(g, h->dt, &r.flops, &r.bytes);
                return r;
            },
            [&] { return launch_gemm(g, h->dt, s); });
    }

    // ---- GemmArgs, one builder per kind: a walk's linear / conv3 starts from these and sets only what is its own ------------------
    // out[M][N] = a[M][K] w[N][K]^T + bias (+ residual), rows of N
    static GemmArgs linear_args(const void* a, int K, const void* w, const float* bias, const void* residual, void* out, int M, int N) {
        GemmArgs g;
        g.A0 = a; g.C0 = K; g.mode = GEMM_LINEAR; g.M = M; g.N = N; g.K = K; g.W = w; g.bias = bias;
        g.epi = residual ? EPI_RESIDUAL : EPI_NONE; g.residual = residual; g.out = out; g.ldo = N;
        return g;
    }
    // 3x3 conv of x to Cout channels.  Output side: twice the input's behind the folded nearest-2x upsample; at stride 2, padding 1
    // (the U-Net's downsamplers) (H - 1) / 2 + 1 = ceil(H / 2) rows (odd sides: --image_size 224 -> 28 -> 14 -> 7 -> 4), with the
    // VAE's right / bottom padding only (pad = 0) H / 2
    static GemmArgs conv3_args(const Act& x, const void* w, const float* bias, const void* residual, void* out, int Cout, int stride,
                               int ups, int pad) {
        const auto side = [&](int n) { return ups ? 2 * n : stride == 2 ? (pad ? (n + 1) / 2 : n / 2) : n; };
        GemmArgs g;
        g.A0 = x.p; g.C0 = x.C; g.mode = GEMM_CONV3; g.Hin = x.H; g.Win = x.W; g.Hout = side(x.H); g.Wout = side(x.W);
        g.stride = stride; g.ups = ups; g.pad = pad;
        g.M = x.B * g.Hout * g.Wout; g.N = Cout; g.K = 9 * x.C; g.W = w; g.bias = bias;
        g.epi = residual ? EPI_RESIDUAL : EPI_NONE; g.residual = residual; g.out = out; g.ldo = Cout;
        return g;
    }
};

}  // namespace

// Repack every raw parameter into the engine's layouts.
// ---- weight packing (finalize) ---------------------------------------------------------------
static inline int pack_all(WeightStore* h, hipStream_t s) {
    const int dt = h->dt;
    const size_t es = dtype_size(dt);
    for (auto& kv : h->raw) {
        const std::string& key = kv.first;
        const RawW& w = kv.second;
        Packed P;
        const bool keep_f32 = key == "pos_embed" || ends_with(key, "x_embedder.proj.weight") ||
                              ends_with(key, "embedding_table.weight") || key.rfind("t_embedder.", 0) == 0 ||
                              ends_with(key, "adaLN_modulation.1.weight");
        if (keep_f32 && w.shape.size() >= 2) {
            // small DiT conditioning tensors consumed by f32 GEMV / lookup / patch-embed kernels: flat f32 copy
            int64_t n = 1;
            for (auto d : w.shape) n *= d;
            CK(h->dalloc((size_t)n * 4, &P.p));
            P.rows = (int)w.shape[0]; P.cols = (int)(n / w.shape[0]); P.bytes = (size_t)n * 4;
            CK(pack_vector(w.p, w.dtype, (float*)P.p, (int)n, 0, s));
            h->pk[key] = P;
        } else if (w.shape.size() == 1) {
            const int n = (int)w.shape[0];
            const int geglu = ends_with(key, "ff.net.0.proj.bias") ? geglu_block_rows(n) : 0;
            CK(h->dalloc((size_t)n * 4, &P.p));
            P.rows = n; P.cols = 1; P.bytes = (size_t)n * 4;
            CK(pack_vector(w.p, w.dtype, (float*)P.p, n, geglu, s));
            h->pk[key] = P;
        } else if (w.shape.size() == 4 && w.shape[2] == 3) {
            const int co = (int)w.shape[0], ci = (int)w.shape[1];
            if (ends_with(key, "conv_in.weight")) {
                CK(h->dalloc((size_t)co * ci * 9 * 4, &P.p));
                P.rows = 9 * ci; P.cols = co;
                CK(pack_conv_in(w.p, w.dtype, (float*)P.p, co, ci, s));
            } else {
                CK(h->dalloc((size_t)co * ci * 9 * es, &P.p));
                P.rows = co; P.cols = 9 * ci;
                CK(pack_conv3(w.p, w.dtype, P.p, dt, co, ci, s));
            }
            h->pk[key] = P;
        } else if (w.shape.size() == 2 || (w.shape.size() == 4 && w.shape[2] == 1)) {
            const int n = (int)w.shape[0], k = (int)w.shape[1];
            const bool is_q1 = ends_with(key, "attn1.to_q.weight"), is_k1 = ends_with(key, "attn1.to_k.weight"),
                       is_v1 = ends_with(key, "attn1.to_v.weight");
            const bool is_k2 = ends_with(key, "attn2.to_k.weight"), is_v2 = ends_with(key, "attn2.to_v.weight");
            if (is_q1 || is_k1 || is_v1) {
                // fused [3C][C] = [to_q ; to_k ; to_v]
                const std::string fk = key.substr(0, key.size() - strlen("to_q.weight")) + "qkv";
                Packed& F = h->pk[fk];
                if (!F.p) { CK(h->dalloc((size_t)3 * n * k * es, &F.p)); F.rows = 3 * n; F.cols = k; }
                const int slot = is_q1 ? 0 : (is_k1 ? 1 : 2);
                CK(pack_linear(w.p, w.dtype, (char*)F.p + (size_t)slot * n * k * es, dt, n, k, 0, s));
            } else if (is_k2 || is_v2) {
                const std::string fk = key.substr(0, key.size() - strlen("to_k.weight")) + "kv";
                Packed& F = h->pk[fk];
                if (!F.p) { CK(h->dalloc((size_t)2 * n * k * es, &F.p)); F.rows = 2 * n; F.cols = k; }
                CK(pack_linear(w.p, w.dtype, (char*)F.p + (size_t)(is_k2 ? 0 : 1) * n * k * es, dt, n, k, 0, s));
            } else if (ends_with(key, "time_emb_proj.weight") || key.rfind("time_embedding.", 0) == 0 ||
                       key.rfind("add_embedding.", 0) == 0) {
                CK(h->dalloc((size_t)n * k * 4, &P.p));        // kept f32: consumed by the GEMV
                P.rows = n; P.cols = k;
                CK(pack_linear(w.p, w.dtype, P.p, DSIM_F32, n, k, 0, s));
                h->pk[key] = P;
            } else {
                const int geglu = ends_with(key, "ff.net.0.proj.weight") ? geglu_block_rows(n) : 0;
                CK(h->dalloc((size_t)n * k * es, &P.p));
                P.rows = n; P.cols = k;
                CK(pack_linear(w.p, w.dtype, P.p, dt, n, k, geglu, s));
                h->pk[key] = P;
            }
        } else {
            return DSIM_ERR_INVALID;
        }
    }
    return DSIM_OK;
}

}  // namespace dsim
