// The C ABI of libdiffsim_amd that belongs to no executor: version / status text / device count, the fused score tails (pairs,
// matrices, maps, alignments, regions, text attention, region transfer) with their workspace queries, and the single-operator and launch-plan entry points (dsim_op_*, dsim_*_plan) the
// tests and micro-benchmarks drive.  The executors' own groups live beside their walks: dsim_unet_* in unet.hip, dsim_vae_* in
// vae.hip, dsim_dit_* in dit.hip.
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

#include "common.h"
#include "store.h"

using namespace dsim;

extern "C" {

int dsim_version(void) { return DSIM_ABI_VERSION; }

const char* dsim_strerror(int st) {
    switch (st) {
        case DSIM_OK: return "ok";
        case DSIM_ERR_INVALID: return "invalid argument or unsupported shape";
        case DSIM_ERR_MISSING_WEIGHT: return "a parameter needed before the tap was never loaded";
        case DSIM_ERR_WORKSPACE: return "workspace too small";
        case DSIM_ERR_HIP: return "HIP runtime error";
        case DSIM_ERR_STATE: return "call order violated";
        case DSIM_ERR_NO_DEVICE: return "no HIP device";
        default: return "unknown status";
    }
}

int dsim_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- the score tails ----
// A workspace query adds 256 bytes to what the launcher asks for (0 stays 0: the call is not served), and an entry point's prologue
// spends them: no required pointer NULL and no refusal of the arguments themselves (DSIM_ERR_INVALID), then the workspace aligned
// up to 256 bytes inside that slack (DSIM_ERR_WORKSPACE).  The launchers repeat the argument checks: they are entry points too.
static size_t with_slack(size_t bytes) { return bytes ? bytes + 256 : 0; }
static int tail_prologue(std::initializer_list<const void*> required, int refusal, void*& workspace, size_t& workspace_bytes) {
    for (const void* p : required)
        if (!p) return DSIM_ERR_INVALID;
    if (!workspace || refusal != DSIM_OK) return DSIM_ERR_INVALID;
    return align_workspace(workspace, workspace_bytes) ? DSIM_OK : DSIM_ERR_WORKSPACE;
}

size_t dsim_pair_score_workspace_bytes(int n_pairs, int B, int H, int N, int D) {
    return pair_score_scratch_bytes(n_pairs, B, H, N, D) + 256;
}

// status may be NULL here; dsim_pair_score_status requires it.  (tiled = false: whether B*H rides on a grid axis is the launcher's to say)
static int pair_score(PairArgs a, int dtype, float* out_scores, int32_t* status, void* stream) {
    const int st = tail_prologue({a.q, a.k, a.v, a.idx_a, a.idx_b, out_scores}, pair_args_check(a, dtype, false), a.scratch, a.scratch_bytes);
    return st != DSIM_OK ? st : launch_pair_score(a, dtype, out_scores, status, (hipStream_t)stream);
}

int dsim_pair_score(const void* q, const void* k, const void* v, const int32_t* idx_a, const int32_t* idx_b, int n_pairs,
                    int B, int H, int N, int D, int dtype, int similarity, float* out_scores, void* workspace,
                    size_t workspace_bytes, void* stream) {
    return pair_score({q, k, v, idx_a, idx_b, n_pairs, B, H, N, D, similarity, workspace, workspace_bytes}, dtype, out_scores, nullptr, stream);
}

int dsim_pair_score_status(const void* q, const void* k, const void* v, const int32_t* idx_a, const int32_t* idx_b,
                           int n_pairs, int B, int H, int N, int D, int dtype, int similarity, float* out_scores,
                           int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (!status) return DSIM_ERR_INVALID;
    return pair_score({q, k, v, idx_a, idx_b, n_pairs, B, H, N, D, similarity, workspace, workspace_bytes}, dtype, out_scores, status, stream);
}

size_t dsim_score_matrix_workspace_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    return with_slack(score_matrix_scratch_bytes(n_a, n_b, B, H, N, D, dtype));
}

int dsim_score_matrix(const void* qa, const void* ka, const void* va, int n_a, const void* qb, const void* kb, const void* vb, int n_b,
                      int B, int H, int N, int D, int dtype, int similarity, float* out, int32_t* status, void* workspace,
                      size_t workspace_bytes, void* stream) {
    MatrixArgs a{{qa, qb}, {ka, kb}, {va, vb}, {nullptr, nullptr}, n_a, n_b, B, H, N, D, similarity, workspace, workspace_bytes};
    const int st = tail_prologue({qa, ka, va, qb, kb, vb, out}, matrix_args_check(a, dtype, false), a.scratch, a.scratch_bytes);
    return st != DSIM_OK ? st : launch_score_matrix(a, dtype, out, status, (hipStream_t)stream);
}

size_t dsim_pair_score_maps_workspace_bytes(int n_pairs, int B, int H, int N, int D) {
    return D >= 1 ? with_slack(pair_score_maps_scratch_bytes(n_pairs, B, H, N)) : 0;
}

int dsim_pair_score_maps(const void* q, const void* k, const void* v, const int32_t* idx_a, const int32_t* idx_b, int n_pairs, int B,
                         int H, int N, int D, int dtype, int similarity, float* score, float* local, float* contrib, int32_t* status,
                         void* workspace, size_t workspace_bytes, void* stream) {
    PairArgs a{q, k, v, idx_a, idx_b, n_pairs, B, H, N, D, similarity, workspace, workspace_bytes};
    const int st = tail_prologue({q, k, v, idx_a, idx_b, score}, pair_args_check(a, dtype), a.scratch, a.scratch_bytes);
    return st != DSIM_OK ? st : launch_pair_score_maps(a, dtype, score, local, contrib, status, (hipStream_t)stream);
}

size_t dsim_pair_score_regions_workspace_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    return with_slack(pair_score_regions_scratch_bytes(n_feat, n_pairs, B, H, N, D));
}

int dsim_pair_score_regions(const void* q, const void* k, const void* v, const uint8_t* mask, int n_feat, const int32_t* idx_a,
                            const int32_t* idx_b, int n_pairs, int B, int H, int N, int D, int dtype, int similarity, float* out_scores,
                            int32_t* status, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    PairArgs a{q, k, v, idx_a, idx_b, n_pairs, B, H, N, D, similarity, workspace, workspace_bytes};
    const bool served = pair_score_regions_scratch_bytes(n_feat, n_pairs, B, H, N, D) != 0;
    const int st = tail_prologue({q, k, v, mask, idx_a, idx_b, out_scores}, served ? pair_args_check(a, dtype) : DSIM_ERR_INVALID, a.scratch,
                                 a.scratch_bytes);
    return st != DSIM_OK ? st : launch_pair_score_regions(a, dtype, mask, n_feat, out_scores, status, counts, (hipStream_t)stream);
}

size_t dsim_pair_score_weights_workspace_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    return with_slack(pair_score_weights_scratch_bytes(n_feat, n_pairs, B, H, N, D));
}

int dsim_pair_score_weights(const void* q, const void* k, const void* v, const uint8_t* weights, int n_feat, const int32_t* idx_a,
                            const int32_t* idx_b, int n_pairs, int B, int H, int N, int D, int dtype, int similarity, float* out_scores,
                            int32_t* status, int32_t* weight_sums, void* workspace, size_t workspace_bytes, void* stream) {
    PairArgs a{q, k, v, idx_a, idx_b, n_pairs, B, H, N, D, similarity, workspace, workspace_bytes};
    const bool served = pair_score_weights_scratch_bytes(n_feat, n_pairs, B, H, N, D) != 0;
    const int st = tail_prologue({q, k, v, weights, idx_a, idx_b, out_scores}, served ? pair_args_check(a, dtype) : DSIM_ERR_INVALID,
                                 a.scratch, a.scratch_bytes);
    return st != DSIM_OK ? st : launch_pair_score_weights(a, dtype, weights, n_feat, out_scores, status, weight_sums, (hipStream_t)stream);
}

size_t dsim_pair_score_maps_regions_workspace_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    return with_slack(pair_score_maps_regions_scratch_bytes(n_feat, n_pairs, B, H, N, D));
}

int dsim_pair_score_maps_regions(const void* q, const void* k, const void* v, const uint8_t* mask, int n_feat, const int32_t* idx_a,
                                 const int32_t* idx_b, int n_pairs, int B, int H, int N, int D, int dtype, int similarity, float* score,
                                 float* local, float* contrib, int32_t* status, int32_t* counts, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    PairArgs a{q, k, v, idx_a, idx_b, n_pairs, B, H, N, D, similarity, workspace, workspace_bytes};
    const bool served = pair_score_maps_regions_scratch_bytes(n_feat, n_pairs, B, H, N, D) != 0;
    const int st = tail_prologue({q, k, v, mask, idx_a, idx_b, score}, served ? pair_args_check(a, dtype) : DSIM_ERR_INVALID, a.scratch,
                                 a.scratch_bytes);
    return st != DSIM_OK ? st
                         : launch_pair_score_maps_regions(a, dtype, mask, n_feat, score, local, contrib, status, counts, (hipStream_t)stream);
}

size_t dsim_pair_align_regions_workspace_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    return with_slack(pair_align_regions_scratch_bytes(n_feat, n_pairs, B, H, N, D));
}

int dsim_pair_align_regions(const void* q, const void* k, const uint8_t* mask, int n_feat, const int32_t* idx_a, const int32_t* idx_b,
                            int n_pairs, int B, int H, int N, int D, int dtype, int grid_w, int32_t* match, float* weight, float* expect,
                            float* attn, int32_t* status, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    PairArgs a{q, k, nullptr, idx_a, idx_b, n_pairs, B, H, N, D, 0, workspace, workspace_bytes};
    const bool served = pair_align_regions_scratch_bytes(n_feat, n_pairs, B, H, N, D) != 0;
    const int st = tail_prologue({q, k, mask, idx_a, idx_b}, served ? pair_args_check(a, dtype) : DSIM_ERR_INVALID, a.scratch, a.scratch_bytes);
    return st != DSIM_OK ? st
                         : launch_pair_align_regions(a, dtype, mask, n_feat, grid_w, match, weight, expect, attn, status, counts,
                                                     (hipStream_t)stream);
}

size_t dsim_score_matrix_regions_workspace_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    return with_slack(score_matrix_regions_scratch_bytes(n_a, n_b, B, H, N, D, dtype));
}

int dsim_score_matrix_regions(const void* qa, const void* ka, const void* va, const uint8_t* mask_a, int n_a, const void* qb,
                              const void* kb, const void* vb, const uint8_t* mask_b, int n_b, int B, int H, int N, int D, int dtype,
                              int similarity, float* out, int32_t* status, int32_t* counts, void* workspace, size_t workspace_bytes,
                              void* stream) {
    MatrixArgs a{{qa, qb}, {ka, kb}, {va, vb}, {mask_a, mask_b}, n_a, n_b, B, H, N, D, similarity, workspace, workspace_bytes};
    const int st = tail_prologue({qa, ka, va, mask_a, qb, kb, vb, mask_b, out}, matrix_args_check(a, dtype, true), a.scratch, a.scratch_bytes);
    return st != DSIM_OK ? st : launch_score_matrix_regions(a, dtype, out, status, counts, (hipStream_t)stream);
}

size_t dsim_pair_score_maps_weights_workspace_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    return with_slack(pair_score_maps_weights_scratch_bytes(n_feat, n_pairs, B, H, N, D));
}

int dsim_pair_score_maps_weights(const void* q, const void* k, const void* v, const uint8_t* weights, int n_feat, const int32_t* idx_a,
                                 const int32_t* idx_b, int n_pairs, int B, int H, int N, int D, int dtype, int similarity, float* score,
                                 float* local, float* contrib, int32_t* status, int32_t* weight_sums, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    PairArgs a{q, k, v, idx_a, idx_b, n_pairs, B, H, N, D, similarity, workspace, workspace_bytes};
    const bool served = pair_score_maps_weights_scratch_bytes(n_feat, n_pairs, B, H, N, D) != 0;
    const int st = tail_prologue({q, k, v, weights, idx_a, idx_b, score}, served ? pair_args_check(a, dtype) : DSIM_ERR_INVALID, a.scratch,
                                 a.scratch_bytes);
    return st != DSIM_OK ? st
                         : launch_pair_score_maps_weights(a, dtype, weights, n_feat, score, local, contrib, status, weight_sums,
                                                          (hipStream_t)stream);
}

size_t dsim_pair_align_weights_workspace_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    return with_slack(pair_align_weights_scratch_bytes(n_feat, n_pairs, B, H, N, D));
}

int dsim_pair_align_weights(const void* q, const void* k, const uint8_t* weights, int n_feat, const int32_t* idx_a, const int32_t* idx_b,
                            int n_pairs, int B, int H, int N, int D, int dtype, int grid_w, int32_t* match, float* weight, float* expect,
                            float* attn, int32_t* status, int32_t* weight_sums, void* workspace, size_t workspace_bytes, void* stream) {
    PairArgs a{q, k, nullptr, idx_a, idx_b, n_pairs, B, H, N, D, 0, workspace, workspace_bytes};
    const bool served = pair_align_weights_scratch_bytes(n_feat, n_pairs, B, H, N, D) != 0;
    const int st = tail_prologue({q, k, weights, idx_a, idx_b}, served ? pair_args_check(a, dtype) : DSIM_ERR_INVALID, a.scratch,
                                 a.scratch_bytes);
    return st != DSIM_OK ? st
                         : launch_pair_align_weights(a, dtype, weights, n_feat, grid_w, match, weight, expect, attn, status, weight_sums,
                                                     (hipStream_t)stream);
}

size_t dsim_score_matrix_weights_workspace_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    return with_slack(score_matrix_weights_scratch_bytes(n_a, n_b, B, H, N, D, dtype));
}

int dsim_score_matrix_weights(const void* qa, const void* ka, const void* va, const uint8_t* weights_a, int n_a, const void* qb,
                              const void* kb, const void* vb, const uint8_t* weights_b, int n_b, int B, int H, int N, int D, int dtype,
                              int similarity, float* out, int32_t* status, int32_t* weight_sums, void* workspace, size_t workspace_bytes,
                              void* stream) {
    MatrixArgs a{{qa, qb}, {ka, kb}, {va, vb}, {weights_a, weights_b}, n_a, n_b, B, H, N, D, similarity, workspace, workspace_bytes};
    const bool served = score_matrix_weights_scratch_bytes(n_a, n_b, B, H, N, D, dtype) != 0;
    const int st = tail_prologue({qa, ka, va, weights_a, qb, kb, vb, weights_b, out},
                                 served ? matrix_args_check(a, dtype, true) : DSIM_ERR_INVALID, a.scratch, a.scratch_bytes);
    return st != DSIM_OK ? st : launch_score_matrix_weights(a, dtype, out, status, weight_sums, (hipStream_t)stream);
}

size_t dsim_pair_align_workspace_bytes(int n_pairs, int B, int H, int N, int D) {
    return with_slack(pair_align_scratch_bytes(n_pairs, B, H, N, D));
}

int dsim_pair_align(const void* q, const void* k, const int32_t* idx_a, const int32_t* idx_b, int n_pairs, int B, int H, int N, int D,
                    int dtype, int grid_w, int32_t* match, float* weight, float* expect, float* attn, int32_t* status, void* workspace,
                    size_t workspace_bytes, void* stream) {
    PairArgs a{q, k, nullptr, idx_a, idx_b, n_pairs, B, H, N, D, 0, workspace, workspace_bytes};
    const int st = tail_prologue({q, k, idx_a, idx_b}, pair_args_check(a, dtype), a.scratch, a.scratch_bytes);
    return st != DSIM_OK ? st : launch_pair_align(a, dtype, grid_w, match, weight, expect, attn, status, (hipStream_t)stream);
}

size_t dsim_pair_region_transfer_workspace_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    return with_slack(pair_region_transfer_scratch_bytes(n_feat, n_pairs, B, H, N, D));
}

int dsim_pair_region_transfer(const void* q, const void* k, const uint8_t* weights, int n_feat, const int32_t* idx_a, const int32_t* idx_b,
                              int n_pairs, int B, int H, int N, int D, int dtype, int directions, float* mass, int32_t* status,
                              void* workspace, size_t workspace_bytes, void* stream) {
    PairArgs a{q, k, nullptr, idx_a, idx_b, n_pairs, B, H, N, D, 0, workspace, workspace_bytes};
    const bool served = pair_region_transfer_scratch_bytes(n_feat, n_pairs, B, H, N, D) != 0 && directions >= 1 && directions <= 3;
    const int st = tail_prologue({q, k, weights, idx_a, idx_b, mass}, served ? pair_args_check(a, dtype) : DSIM_ERR_INVALID, a.scratch,
                                 a.scratch_bytes);
    return st != DSIM_OK ? st : launch_pair_region_transfer(a, dtype, weights, n_feat, directions, mass, status, (hipStream_t)stream);
}

size_t dsim_region_transfer_matrix_workspace_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    return with_slack(region_transfer_matrix_scratch_bytes(n_a, n_b, B, H, N, D, dtype));
}

int dsim_region_transfer_matrix(const void* qa, const void* ka, const uint8_t* weights_a, int n_a, const void* qb, const void* kb, int n_b,
                                int B, int H, int N, int D, int dtype, float* mass, int32_t* status, void* workspace, size_t workspace_bytes,
                                void* stream) {
    MatrixArgs a{{qa, qb}, {ka, kb}, {nullptr, nullptr}, {weights_a, nullptr}, n_a, n_b, B, H, N, D, 0, workspace, workspace_bytes};
    const bool served = region_transfer_matrix_scratch_bytes(n_a, n_b, B, H, N, D, dtype) != 0;
    const int st = tail_prologue({qa, ka, weights_a, qb, kb, mass}, served ? DSIM_OK : DSIM_ERR_INVALID, a.scratch, a.scratch_bytes);
    return st != DSIM_OK ? st : launch_region_transfer_matrix(a, dtype, mass, status, (hipStream_t)stream);
}

size_t dsim_score_matrix_cell_regions_workspace_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    return with_slack(score_matrix_cell_regions_scratch_bytes(n_a, n_b, B, H, N, D, dtype));
}

int dsim_score_matrix_cell_regions(const void* qa, const void* ka, const void* va, const uint8_t* mask_a, int n_a, const void* qb,
                                   const void* kb, const void* vb, const uint8_t* mask_b, int n_b, int B, int H, int N, int D, int dtype,
                                   int similarity, float* out, int32_t* status, int32_t* counts, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    MatrixArgs a{{qa, qb}, {ka, kb}, {va, vb}, {mask_a, mask_b}, n_a, n_b, B, H, N, D, similarity, workspace, workspace_bytes};
    const bool served = score_matrix_cell_regions_scratch_bytes(n_a, n_b, B, H, N, D, dtype) != 0 && (similarity == 0 || similarity == 1);
    const int st = tail_prologue({qa, ka, va, mask_a, qb, kb, vb, mask_b, out}, served ? DSIM_OK : DSIM_ERR_INVALID, a.scratch, a.scratch_bytes);
    return st != DSIM_OK ? st : launch_score_matrix_cell_regions(a, dtype, out, status, counts, (hipStream_t)stream);
}

size_t dsim_score_matrix_cell_weights_workspace_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    return with_slack(score_matrix_cell_weights_scratch_bytes(n_a, n_b, B, H, N, D, dtype));
}

int dsim_score_matrix_cell_weights(const void* qa, const void* ka, const void* va, const uint8_t* weights_a, int n_a, const void* qb,
                                   const void* kb, const void* vb, const uint8_t* weights_b, int n_b, int B, int H, int N, int D, int dtype,
                                   int similarity, float* out, int32_t* status, int32_t* weight_sums, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    MatrixArgs a{{qa, qb}, {ka, kb}, {va, vb}, {weights_a, weights_b}, n_a, n_b, B, H, N, D, similarity, workspace, workspace_bytes};
    const bool served = score_matrix_cell_weights_scratch_bytes(n_a, n_b, B, H, N, D, dtype) != 0 && (similarity == 0 || similarity == 1);
    const int st = tail_prologue({qa, ka, va, weights_a, qb, kb, vb, weights_b, out}, served ? DSIM_OK : DSIM_ERR_INVALID, a.scratch,
                                 a.scratch_bytes);
    return st != DSIM_OK ? st : launch_score_matrix_cell_weights(a, dtype, out, status, weight_sums, (hipStream_t)stream);
}

size_t dsim_text_attention_workspace_bytes(int n_images, int N, int L) { return with_slack(text_attention_scratch_bytes(n_images, N, L)); }

int dsim_text_attention(const void* xq, int ldq, const void* xk, int ldk, int n_images, int n_kv, int H, int N, int L, int D, int dtype,
                        const float* token_weight, int n_w, float rel_threshold, float* attn, float* saliency, uint8_t* mask,
                        int32_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const int st = tail_prologue({xq, xk}, text_attention_scratch_bytes(n_images, N, L) ? DSIM_OK : DSIM_ERR_INVALID, workspace,
                                 workspace_bytes);
    if (st != DSIM_OK) return st;
    return launch_text_attention(xq, ldq, xk, ldk, n_images, n_kv, H, N, L, D, dtype, token_weight, n_w, rel_threshold, attn, saliency,
                                 mask, counts, status, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- single-operator entry points (tests / micro-benchmarks; these allocate and synchronise) ----
namespace {
struct Tmp {
    std::vector<void*> v;
    ~Tmp() { for (void* p : v) (void)hipFree(p); }
    void* get(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr;
        v.push_back(p);
        return p;
    }
};
}  // namespace

int dsim_op_linear(const void* x, const float* w, const float* bias, const void* residual, void* out, int M, int N,
                   int K, int dtype, int geglu, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    Tmp t;
    const int NW = geglu ? 2 * N : N;
    void* wp = t.get((size_t)NW * K * dtype_size(dtype));
    float* bp = bias ? (float*)t.get((size_t)NW * 4) : nullptr;
    void* zp = t.get(256);
    if (!wp || !zp || (bias && !bp)) return DSIM_ERR_HIP;
    DSIM_HIP_CHECK(hipMemsetAsync(zp, 0, 256, s));
    const int gblk = geglu ? geglu_block_rows(NW) : 0;
    CK(pack_linear(w, DSIM_F32, wp, dtype, NW, K, gblk, s));
    if (bias) CK(pack_vector(bias, DSIM_F32, bp, NW, gblk, s));
    GemmArgs g;
    g.A0 = x; g.C0 = K; g.mode = GEMM_LINEAR; g.M = M; g.N = NW; g.K = K; g.W = wp; g.bias = bp;
    g.epi = geglu ? EPI_GEGLU : (residual ? EPI_RESIDUAL : EPI_NONE);
    if (geglu) g.geglu_blk = gblk;
    g.residual = residual; g.out = out; g.ldo = N; g.zero_page = zp;
    CK(launch_gemm(g, dtype, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    return DSIM_OK;
}

int dsim_op_conv3x3(const void* x, const float* w, const float* bias, const void* residual, void* out, int B, int H,
                    int W, int Cin, int Cout, int stride, int upsample, int dtype, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    Tmp t;
    void* wp = t.get((size_t)Cout * 9 * Cin * dtype_size(dtype));
    void* zp = t.get(256);
    if (!wp || !zp) return DSIM_ERR_HIP;
    DSIM_HIP_CHECK(hipMemsetAsync(zp, 0, 256, s));
    CK(pack_conv3(w, DSIM_F32, wp, dtype, Cout, Cin, s));
    GemmArgs g;
    g.A0 = x; g.C0 = Cin; g.mode = GEMM_CONV3; g.Hin = H; g.Win = W;
    g.Hout = upsample ? 2 * H : (stride == 2 ? (H + 1) / 2 : H);      // stride 2, padding 1: ceil(H / 2), as the executor
    g.Wout = upsample ? 2 * W : (stride == 2 ? (W + 1) / 2 : W);
    g.stride = stride; g.ups = upsample ? 1 : 0;
    g.M = B * g.Hout * g.Wout; g.N = Cout; g.K = 9 * Cin; g.W = wp; g.bias = bias;
    g.epi = residual ? EPI_RESIDUAL : EPI_NONE; g.residual = residual; g.out = out; g.ldo = Cout; g.zero_page = zp;
    CK(launch_gemm(g, dtype, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    return DSIM_OK;
}

int dsim_op_gemm(const dsim_gemm_op* op, dsim_gemm_launch* launched, void* stream) {
    if (!op || !launched || !op->A0 || !op->w || !op->out) return DSIM_ERR_INVALID;
    const int dt = op->dtype;
    if ((dt != DSIM_F32 && dt != DSIM_BF16 && dt != DSIM_F16) || (op->mode != GEMM_LINEAR && op->mode != GEMM_CONV3)) return DSIM_ERR_INVALID;
    if (op->M <= 0 || op->N <= 0 || op->K <= 0 || op->wb_rows < 0) return DSIM_ERR_INVALID;
    if ((op->bias2 || op->gate2) && op->rows_per_batch <= 0) return DSIM_ERR_INVALID;
    if ((op->bias2 && !op->bias) || (op->gate2 && !op->gate)) return DSIM_ERR_INVALID;      // the odd rows' vector replaces the even rows'
    {
        // rows are ldo elements apart: at least the columns one output tensor receives
        const int ncol = op->epi == EPI_GEGLU ? op->N / 2 : op->N;
        if (op->ldo < (op->out_split > 0 ? op->out_split : ncol)) return DSIM_ERR_INVALID;
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t es = dtype_size(dt);
    const bool geglu = op->epi == EPI_GEGLU;
    GemmArgs g;
    g.A0 = op->A0; g.C0 = op->C0; g.A1 = op->A1; g.C1 = op->A1 ? op->C1 : 0;
    g.mode = op->mode; g.M = op->M; g.N = op->N; g.K = op->K;
    if (op->mode == GEMM_CONV3) {
        if (op->pad != 0 && op->pad != 1) return DSIM_ERR_INVALID;
        if (op->pad == 0 && (op->stride != 2 || op->ups)) return DSIM_ERR_INVALID;      // the VAE downsample's form only
        g.Hin = op->H; g.Win = op->W; g.stride = op->stride; g.ups = op->ups ? 1 : 0; g.pad = op->pad;
        // stride 2: ceil(H / 2) rows with padding 1, H / 2 with the right / bottom padding of the VAE (pad 0)
        g.Hout = op->ups ? 2 * op->H : (op->stride == 2 ? (op->pad ? (op->H + 1) / 2 : op->H / 2) : op->H);
        g.Wout = op->ups ? 2 * op->W : (op->stride == 2 ? (op->pad ? (op->W + 1) / 2 : op->W / 2) : op->W);
        if (g.Hout <= 0 || g.Wout <= 0 || op->M % (g.Hout * g.Wout)) return DSIM_ERR_INVALID;
    }
    const int gblk = geglu ? geglu_block_rows(op->N) : 0;
    const int nmat = op->wb_rows > 0 ? op->M / op->wb_rows : 1;
    const size_t wmat = (size_t)op->N * op->K * es;
    if (op->wb_rows > 0 && (op->M % op->wb_rows || op->wb_stride % 16 || (size_t)op->wb_stride < wmat)) return DSIM_ERR_INVALID;
    Tmp t;
    void* wp = t.get(op->wb_rows > 0 ? (size_t)(nmat - 1) * op->wb_stride + wmat : wmat);
    float* bp = op->bias ? (float*)t.get((size_t)op->N * 4) : nullptr;
    float* b2p = op->bias2 ? (float*)t.get((size_t)op->N * 4) : nullptr;
    void* zp = t.get(256);
    if (!wp || !zp || (op->bias && !bp) || (op->bias2 && !b2p)) return DSIM_ERR_HIP;
    DSIM_HIP_CHECK(hipMemsetAsync(zp, 0, 256, s));
    if (op->mode == GEMM_CONV3) {
        CK(pack_conv3(op->w, DSIM_F32, wp, dt, op->N, op->C0, s));
    } else {
        for (int i = 0; i < nmat; ++i)
            CK(pack_linear(op->w + (size_t)i * op->N * op->K, DSIM_F32, (char*)wp + (size_t)i * op->wb_stride, dt, op->N, op->K, gblk, s));
    }
    if (op->bias) CK(pack_vector(op->bias, DSIM_F32, bp, op->N, gblk, s));
    if (op->bias2) CK(pack_vector(op->bias2, DSIM_F32, b2p, op->N, gblk, s));
    g.W = wp; g.bias = bp; g.bias2 = b2p; g.rows_per_batch = op->rows_per_batch;
    g.act = op->act; g.gate = op->gate; g.gate2 = op->gate2;
    g.epi = op->epi;
    if (geglu) g.geglu_blk = gblk;
    g.residual = op->residual; g.out = op->out; g.ldo = op->ldo;
    g.out_split = op->out_split; g.out_split_stride = op->out_split_stride;
    g.force_big = op->force_big;
    g.wb_rows = op->wb_rows; g.wb_stride = op->wb_rows > 0 ? op->wb_stride : 0;
    g.gn_part = op->gn_part; g.gn_hw = op->gn_hw;
    g.zero_page = zp;
    double fl = 0, by = 0;
    const std::string fam = gemm_family(g, dt, &fl, &by);
    g_gemm_last_launch = GemmLaunchRec{};
    CK(launch_gemm(g, dt, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    const GemmLaunchRec& r = g_gemm_last_launch;
    launched->bm = r.bm; launched->bn = r.bn; launched->kind = r.mode; launched->geglu = r.geglu; launched->ek = r.ek;
    launched->small = r.small;
    std::snprintf(launched->family, sizeof(launched->family), "%s", fam.c_str());
    return DSIM_OK;
}

int dsim_op_groupnorm_pre(const void* x, int C, const float* gamma, const float* beta, void* out, int B, int HW, int groups,
                          float eps, int silu, int dtype, const float* part32, int chunks, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!x || !gamma || !beta || !out || !part32 || B <= 0 || HW <= 0 || groups <= 0 || C % groups) return DSIM_ERR_INVALID;
    if (chunks < 1 || (long)chunks * 64 != HW) return DSIM_ERR_INVALID;        // one partial per 64 rows of each image (gn_part's layout)
    Tmp t;
    void* sc = t.get(groupnorm_scratch_bytes(B, groups));
    if (!sc) return DSIM_ERR_HIP;
    CK(launch_groupnorm_pre(x, C, gamma, beta, out, B, HW, groups, eps, silu, dtype, sc, part32, chunks, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    return DSIM_OK;
}

int dsim_op_groupnorm(const void* x0, int C0, const void* x1, int C1, const float* gamma, const float* beta, void* out,
                      int B, int HW, int groups, float eps, int silu, int dtype, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    Tmp t;
    void* sc = t.get(groupnorm_scratch_bytes(B, groups));
    if (!sc) return DSIM_ERR_HIP;
    CK(launch_groupnorm(x0, C0, x1, C1, gamma, beta, out, B, HW, groups, eps, silu, dtype, sc, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    return DSIM_OK;
}

int dsim_op_layernorm(const void* x, const float* gamma, const float* beta, void* out, int M, int C, float eps, int dtype,
                      void* stream) {
    hipStream_t s = (hipStream_t)stream;
    CK(launch_layernorm(x, gamma, beta, out, M, C, eps, dtype, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    return DSIM_OK;
}

int dsim_op_layernorm_mod(const void* x, const float* scale2, const float* shift2, void* out, int M, int C, int rows_per_batch,
                          float eps, int dtype, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!x || !scale2 || !shift2 || !out) return DSIM_ERR_INVALID;
    CK(launch_layernorm_mod(x, scale2, shift2, out, M, C, rows_per_batch, eps, dtype, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    return DSIM_OK;
}

int dsim_groupnorm_plan(int C0, int C1, int B, int HW, int groups, int dtype, int pre, dsim_gn_plan* plan) {
    return groupnorm_plan(C0, C1, B, HW, groups, dtype, pre, plan);
}

int dsim_layernorm_plan(int M, int C, int dtype, int mod, dsim_ln_plan* plan) { return layernorm_plan(M, C, dtype, mod, plan); }

int dsim_op_ff_fused_dt(const void* x, const float* ln_gamma, const float* ln_beta, const float* w1, const float* b1,
                        const float* w2, const float* b2, void* out, int M, int C, float eps, int dtype, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const size_t sb = ff_stream_bytes(C);
    if ((dtype != DSIM_BF16 && dtype != DSIM_F16) || !sb || !x || !out || !w1 || !b1 || !w2 || !b2 || !ln_gamma || !ln_beta) return DSIM_ERR_INVALID;
    Tmp t;
    void* w1p = t.get((size_t)8 * C * C * 2);
    float* b1p = (float*)t.get((size_t)8 * C * 4);
    void* w2p = t.get((size_t)4 * C * C * 2);
    void* st = t.get(sb);
    if (!w1p || !b1p || !w2p || !st) return DSIM_ERR_HIP;
    CK(pack_linear(w1, DSIM_F32, w1p, dtype, 8 * C, C, 32, s));
    CK(pack_vector(b1, DSIM_F32, b1p, 8 * C, 32, s));
    CK(pack_linear(w2, DSIM_F32, w2p, dtype, C, 4 * C, 0, s));
    CK(pack_ff_stream(w1p, w2p, st, C, s));
    FFArgs a;
    a.x = x; a.out = out; a.ln_g = ln_gamma; a.ln_b = ln_beta; a.stream = st; a.b1 = b1p; a.b2 = b2; a.M = M; a.C = C; a.eps = eps; a.dtype = dtype;
    CK(launch_ff_fused(a, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    return DSIM_OK;
}

int dsim_op_ff_fused(const void* x, const float* ln_gamma, const float* ln_beta, const float* w1, const float* b1,
                     const float* w2, const float* b2, void* out, int M, int C, float eps, void* stream) {
    return dsim_op_ff_fused_dt(x, ln_gamma, ln_beta, w1, b1, w2, b2, out, M, C, eps, DSIM_BF16, stream);
}

int dsim_op_ln_linear_dt(const void* x, const float* ln_gamma, const float* ln_beta, const float* w, void* out, int M, int C, int N,
                         float eps, int dtype, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const size_t sb = rowlin_stream_bytes(C, N);
    if ((dtype != DSIM_BF16 && dtype != DSIM_F16) || !sb || !x || !out || !w || !ln_gamma != !ln_beta) return DSIM_ERR_INVALID;
    Tmp t;
    void* wp = t.get((size_t)N * C * 2);
    void* st = t.get(sb);
    if (!wp || !st) return DSIM_ERR_HIP;
    CK(pack_linear(w, DSIM_F32, wp, dtype, N, C, 0, s));
    CK(pack_rowlin_stream(wp, st, C, N, s));
    RowLinArgs a;
    a.x = x; a.out = out; a.ln_g = ln_gamma; a.ln_b = ln_beta; a.stream = st; a.M = M; a.C = C; a.N = N; a.eps = eps; a.dtype = dtype;
    CK(launch_rowlin(a, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    return DSIM_OK;
}

int dsim_op_gn_linear_dt(const void* x, const float* gamma, const float* beta, int groups, float eps, const float* w, const float* bias,
                         void* out, int B, int HW, int C, int N, int dtype, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const size_t sb = rowlin_stream_bytes(C, N);
    if ((dtype != DSIM_BF16 && dtype != DSIM_F16) || !sb || N > C || !x || !out || !w || !gamma != !beta || B < 1 || HW < 1) return DSIM_ERR_INVALID;
    if (gamma && (groups < 1 || HW % 128)) return DSIM_ERR_INVALID;        // a 128-row tile lies inside one image
    Tmp t;
    void* wp = t.get((size_t)N * C * 2);
    void* st = t.get(sb);
    void* sc = gamma ? t.get(groupnorm_scratch_bytes(B, groups)) : nullptr;
    float* coef = gamma ? (float*)t.get((size_t)B * 2 * C * sizeof(float)) : nullptr;
    if (!wp || !st || (gamma && (!sc || !coef))) return DSIM_ERR_HIP;
    CK(pack_linear(w, DSIM_F32, wp, dtype, N, C, 0, s));
    CK(pack_rowlin_stream(wp, st, C, N, s));
    RowLinArgs a;
    a.x = x; a.out = out; a.stream = st; a.M = B * HW; a.C = C; a.N = N; a.dtype = dtype; a.gn = 1; a.bias = bias; a.HW = HW;
    if (gamma) {
        CK(launch_groupnorm_stats(x, C, gamma, beta, B, HW, groups, eps, dtype, sc, coef, s));
        a.coef = coef;
    }
    CK(launch_rowlin(a, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    return DSIM_OK;
}

int dsim_op_ln_linear(const void* x, const float* ln_gamma, const float* ln_beta, const float* w, void* out, int M, int C, int N,
                      float eps, void* stream) {
    return dsim_op_ln_linear_dt(x, ln_gamma, ln_beta, w, out, M, C, N, eps, DSIM_BF16, stream);
}

int dsim_op_attention(const void* q, int ldq, const void* k, const void* v, int ldk, void* out, int ldo, int B, int Bkv,
                      int H, int Nq, int Nk, int D, int dtype, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    AttnArgs a;
    a.q = q; a.ldq = ldq; a.k = k; a.v = v; a.ldk = ldk; a.out = out; a.ldo = ldo;
    a.B = B; a.Bkv = Bkv; a.H = H; a.Nq = Nq; a.Nk = Nk; a.D = D;
    CK(launch_attention(a, dtype, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    return DSIM_OK;
}

int dsim_op_attention_fp8(const void* q, int ldq, const void* k, const void* v, int ldk, void* out, int ldo, int B, int Bkv,
                          int H, int Nq, int Nk, int D, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    AttnArgs a;
    a.q = q; a.ldq = ldq; a.k = k; a.v = v; a.ldk = ldk; a.out = out; a.ldo = ldo;
    a.B = B; a.Bkv = Bkv; a.H = H; a.Nq = Nq; a.Nk = Nk; a.D = D;
    CK(launch_attention_fp8(a, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    return DSIM_OK;
}

static int attn_fp8_ok(const AttnArgs& a) {
    // launch_attention_fp8's own refusals
    if (!a.q || !a.k || !a.v || !a.out || a.B < 1 || a.Bkv < 1 || a.H < 1 || a.Nq < 1 || a.Nk < 1) return 0;
    return !(a.ldq % 8 || a.ldk % 8 || a.ldo % 4) && (a.D == 72 || a.D == 32);
}

int dsim_attention_plan(const void* q, int ldq, const void* k, const void* v, int ldk, const void* out, int ldo, int B, int Bkv,
                        int H, int Nq, int Nk, int D, int dtype, int fp8, int* kind) {
    if (!kind) return DSIM_ERR_INVALID;
    AttnArgs a;
    a.q = q; a.ldq = ldq; a.k = k; a.v = v; a.ldk = ldk; a.out = (void*)out; a.ldo = ldo;
    a.B = B; a.Bkv = Bkv; a.H = H; a.Nq = Nq; a.Nk = Nk; a.D = D;
    if (fp8) {
        if (dtype != DSIM_BF16 || !attn_fp8_ok(a)) return DSIM_ERR_INVALID;
        *kind = DSIM_ATTN_FP8;
        return DSIM_OK;
    }
    const int r = attention_plan(a, dtype);
    if (r < 0) return r;
    *kind = r;
    return DSIM_OK;
}

int dsim_op_attention_ex(const void* q, int ldq, const void* k, const void* v, int ldk, void* out, int ldo, int B, int Bkv, int H,
                         int Nq, int Nk, int D, int dtype, int fp8, dsim_attn_launch* launched, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    AttnArgs a;
    a.q = q; a.ldq = ldq; a.k = k; a.v = v; a.ldk = ldk; a.out = out; a.ldo = ldo;
    a.B = B; a.Bkv = Bkv; a.H = H; a.Nq = Nq; a.Nk = Nk; a.D = D;
    if (fp8 && dtype != DSIM_BF16) return DSIM_ERR_INVALID;
    g_attn_last_launch = AttnLaunchRec{};
    CK(fp8 ? launch_attention_fp8(a, s) : launch_attention(a, dtype, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    if (launched) {
        const AttnLaunchRec& r = g_attn_last_launch;
        launched->kind = r.kind; launched->D = r.D; launched->dtype = r.dtype; launched->k80 = r.k80; launched->qit = r.qit;
        launched->grid = r.grid;
        const char* dtn = dtype_name(r.dtype);
        if (r.kind == DSIM_ATTN_FP8) std::snprintf(launched->family, sizeof(launched->family), "attention_fp8_d%d", r.D);
        else std::snprintf(launched->family, sizeof(launched->family), "attention_%s_d%d%s", dtn, r.D, attn_kind_suffix(r.kind));
    }
    return DSIM_OK;
}

int dsim_op_softmax_rows(const void* x, void* out, int rows, int cols, float scale, int dtype, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!x || !out) return DSIM_ERR_INVALID;
    CK(launch_softmax_rows(x, out, rows, cols, scale, dtype, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    return DSIM_OK;
}

// ---- the input, embedding and weight-packing kernels, one operator each (pack.hip, and the shared launch functions of dit.hip / vae.hip) ----
static bool is_dtype(int dt) { return dt == DSIM_F32 || dt == DSIM_BF16 || dt == DSIM_F16; }
static int synced(int st, hipStream_t s) {
    if (st != DSIM_OK) return st;
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    return DSIM_OK;
}

int dsim_op_conv_in(const float* lat, const float* noise, float sa, float sb, const float* w, const float* bias, void* out, int dtype,
                    int n_img, int Cin, int S, int Cout, int dup, float* gn_part, int force, int* kernel, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!lat || !w || !bias || !out || !is_dtype(dtype)) return DSIM_ERR_INVALID;
    if (n_img < 1 || n_img > 65535 || Cin < 1 || S < 1 || S > 32768 || Cout < 1 || (dup != 1 && dup != 2)) return DSIM_ERR_INVALID;
    if (force < 0 || force > CONV_IN_ROWS) return DSIM_ERR_INVALID;
    // the walks' choice: the VAE's row kernel where it applies (no noising, one copy), else prep_conv_in()'s
    const bool rows_ok = conv_in_rows_applies(Cin, S, Cout) && !noise && dup == 1;
    const int kind = force ? force : (rows_ok ? (int)CONV_IN_ROWS : prep_conv_in_kind(Cin, Cout));
    if (kind == CONV_IN_ROWS ? !rows_ok : (gn_part || !prep_conv_in_kind_applies(kind, Cin, Cout))) return DSIM_ERR_INVALID;
    if (kind != CONV_IN_GENERIC && (uintptr_t)bias % 16) return DSIM_ERR_INVALID;       // (read as float4)
    Tmp t;
    float* wp = (float*)t.get((size_t)9 * Cin * Cout * 4);
    if (!wp) return DSIM_ERR_HIP;
    CK(pack_conv_in(w, DSIM_F32, wp, Cout, Cin, s));
    CK(synced(kind == CONV_IN_ROWS ? conv_in_rows(lat, wp, bias, out, dtype, n_img, S, gn_part, s)
                                   : prep_conv_in_as(kind, lat, noise, sa, sb, wp, bias, out, dtype, n_img, Cin, S, Cout, dup, s), s));
    if (kernel) *kernel = kind;
    return DSIM_OK;
}

int dsim_op_timestep_sincos(float* out, int dim, int t, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!out || dim < 2 || dim % 2) return DSIM_ERR_INVALID;
    return synced(timestep_sincos(out, dim, t, s), s);
}

int dsim_op_sincos_values(float* out, int dim, const float* vals, int count, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!out || !vals || dim < 2 || dim % 2 || count < 1 || (long)count * dim > 0x7fffffffL) return DSIM_ERR_INVALID;
    return synced(sincos_values(out, dim, vals, count, s), s);
}

int dsim_op_gemv_f32(const void* W, int w_dtype, const void* bias, int b_dtype, const float* x, float* y, int N, int K, int act,
                     void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!W || !x || !y || N < 1 || K < 1 || !is_dtype(w_dtype) || (bias && !is_dtype(b_dtype)) || (act != 0 && act != 1)) return DSIM_ERR_INVALID;
    return synced(gemv_f32(W, w_dtype, bias, b_dtype, x, y, N, K, act, s), s);
}

int dsim_op_pack(int kind, const void* src, int src_dtype, void* dst, int dst_dtype, int rows, int cols, int geglu, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!src || !dst || !is_dtype(src_dtype) || !is_dtype(dst_dtype) || rows < 1 || cols < 1) return DSIM_ERR_INVALID;
    const bool f32_only = kind == DSIM_PACK_CONV_IN || kind == DSIM_PACK_VECTOR, interleaves = kind == DSIM_PACK_LINEAR || kind == DSIM_PACK_VECTOR;
    if ((f32_only && dst_dtype != DSIM_F32) || (!interleaves && geglu)) return DSIM_ERR_INVALID;
    if (geglu && ((geglu != 16 && geglu != 32) || rows % (2 * geglu))) return DSIM_ERR_INVALID;
    switch (kind) {
        case DSIM_PACK_LINEAR: return synced(pack_linear(src, src_dtype, dst, dst_dtype, rows, cols, geglu, s), s);
        case DSIM_PACK_CONV3: return synced(pack_conv3(src, src_dtype, dst, dst_dtype, rows, cols, s), s);
        case DSIM_PACK_CONV_IN: return synced(pack_conv_in(src, src_dtype, (float*)dst, rows, cols, s), s);
        case DSIM_PACK_VECTOR: return cols != 1 ? DSIM_ERR_INVALID : synced(pack_vector(src, src_dtype, (float*)dst, rows, geglu, s), s);
    }
    return DSIM_ERR_INVALID;
}

int dsim_op_dup_batch(const void* in, void* out, int n_batch, size_t bytes_per_elem, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!in || !out || n_batch < 1 || !bytes_per_elem) return DSIM_ERR_INVALID;
    return synced(dup_batch(in, out, n_batch, bytes_per_elem, s), s);
}

int dsim_op_resize_nearest(const void* in, void* out, int B, int Hin, int Win, int Hout, int Wout, size_t row_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!in || !out || !row_bytes) return DSIM_ERR_INVALID;
    return synced(resize_nearest(in, out, B, Hin, Win, Hout, Wout, row_bytes, s), s);
}

int dsim_op_gather_ctx(const float* ctx, int n_ctx, const int32_t* index, void* dst, int dtype, int n_images, size_t per, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!is_dtype(dtype)) return DSIM_ERR_INVALID;
    return synced(gather_ctx(ctx, n_ctx, index, dst, dtype, n_images, per, s), s);
}

int dsim_op_patch_embed(const float* lat, const float* noise, float sa, float sb, const float* w, const float* bias, const float* pos,
                        void* out, int dtype, int n_img, int Cin, int S, int p, int D, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    // (the kernel always noises: both lat and noise are read)
    if (!lat || !noise || !w || !bias || !pos || !out || !is_dtype(dtype)) return DSIM_ERR_INVALID;
    if (n_img < 1 || n_img > 65535 || Cin < 1 || p < 1 || S < p || S > 4096 || S % p || D < 1) return DSIM_ERR_INVALID;
    if ((size_t)Cin * p * p * 8 * sizeof(float) > 48 * 1024) return DSIM_ERR_INVALID;            // its staging buffer: 8 tokens x K
    return synced(patch_embed(lat, noise, sa, sb, w, bias, pos, out, dtype, n_img, Cin, S, p, D, s), s);
}

int dsim_op_fold_quant(const float* wq, const void* wco, const float* bco, const float* bq, void* out_w, float* out_b, int Cm, int K,
                       int dtype, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!wq || (!out_w && !out_b) || (out_w && !wco) || (out_b && (!bco || !bq)) || !is_dtype(dtype)) return DSIM_ERR_INVALID;
    return synced(fold_quant(wq, wco, bco, bq, out_w, out_b, Cm, K, dtype, s), s);
}

int dsim_op_to_nchw_f32(const void* x, float* out, int n, int HW, int C, int dtype, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!x || !out || n < 1 || HW < 1 || C < 1 || !is_dtype(dtype)) return DSIM_ERR_INVALID;
    return synced(to_nchw_f32(x, out, n, HW, C, dtype, s), s);
}

}  // extern "C"
