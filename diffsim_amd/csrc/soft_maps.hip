// Soft region maps and soft region alignments: the per-token outputs of the soft region score (soft_regions.hip) and of its biased
// cross-attention.  Every feature image i carries a byte m_i[t] per token, w = m / 255; the tokens of byte 0 are dropped as the region
// forms drop an off token, and a listed key of weight w enters every softmax with the bias ln w (include/diffsim_amd.h,
// dsim_pair_score_maps_weights, dsim_pair_align_weights).  The outputs lie on the full token grid.
//
//   the lists                regions.hip's region_lists_kernel over m != 0
//   soft_weights_kernel      (soft_core.h) the biases by compacted position and the byte sums
//   soft_map_kernel          pair_tail_body, per token, with RowsWeighted: both attends biased as the soft tail's, the per-token
//                            partials UNWEIGHTED (the query weight is the finish's)
//   the map finish           pair_map_finish_kernel<RowsWeighted> (tail_core.h): local is the token's own value; the squared norms and
//                            contrib carry byte / 255 in f64; the mse count is B H D (byte sum) / 255
//   region_align_off_kernel  (region_maps_core.h) over m == 0: the off values and the status word (2: an image of byte sum 0)
//   soft_align_stats_kernel / soft_align_kernel
//                            align_core.h's two passes with RowsWeighted: exp2(fma(s, c, -m c) + lb[j]) with the raw running maximum
// With bytes 0 / 255 every addition is + 0.0f and every factor 1: dsim_pair_score_maps_regions' and dsim_pair_align_regions' bits.
// A translation unit of its own for regions.hip's reason.
#include "region_maps_core.h"
#include "soft_core.h"

namespace dsim {
namespace {

// grid (ceil(N/128), B*H, n_pairs*2).  part: [pair][dir][comp][bh][N] f32 by position
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void soft_map_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                        const T* __restrict__ vg, const int32_t* __restrict__ list,
                                                        const int32_t* __restrict__ cnt, const float* __restrict__ lb,
                                                        const uint8_t* __restrict__ w, int stride, const int32_t* __restrict__ idx_a,
                                                        const int32_t* __restrict__ idx_b, int B, int H, int N,
                                                        float scale_log2, int mse, float* __restrict__ part) {
    pair_tail_body<T, D, true, RowsWeighted>(qg, kg, vg, list, cnt, idx_a, idx_b, B, H, N, scale_log2, mse, part,
                                             RowsWeighted::Table{lb, w, stride});
}

// pass 1 of the alignments over weighted rows.  grid (ceil(N/128), B*H, n_pairs*2); stats [pair][dir][bh][N] float2 by position
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void soft_align_stats_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                           const int32_t* __restrict__ list, const int32_t* __restrict__ cnt,
                                                           const float* __restrict__ lb, int stride, const int32_t* __restrict__ idx_a,
                                                           const int32_t* __restrict__ idx_b, int B, int H, int N, float c,
                                                           float2* __restrict__ stats) {
    align_stats_body<T, D, RowsWeighted>(qg, kg, list, cnt, idx_a, idx_b, B, H, N, c, stats, RowsWeighted::Table{lb, nullptr, stride});
}

// pass 2.  grid (ceil(N/128), n_pairs*2)
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void soft_align_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                     const int32_t* __restrict__ list, const int32_t* __restrict__ cnt,
                                                     const float* __restrict__ lb, int stride, const int32_t* __restrict__ idx_a,
                                                     const int32_t* __restrict__ idx_b, int B, int H, int N, float c, float rbh, int grid_w,
                                                     const float2* __restrict__ stats, int32_t* __restrict__ match,
                                                     float* __restrict__ weight, float* __restrict__ expect, float* __restrict__ attn,
                                                     int32_t* __restrict__ status) {
    align_body<T, D, RowsWeighted>(qg, kg, list, cnt, idx_a, idx_b, B, H, N, c, rbh, grid_w, stats, match, weight, expect, attn, status,
                                   RowsWeighted::Table{lb, nullptr, stride});
}

// workspace: [lists | counts | biases f32 [n_feat][stride] | byte sums int32 [n_feat] | the call's partials or statistics]
struct SoftLayout {
    RegionLayout R;
    size_t bias, sums;
    SoftLayout(int n_feat, int N) : R(n_feat, N), bias(soft_bias_bytes(n_feat, N)), sums(soft_count_bytes(n_feat)) {}
    float* lb(void* ws) const { return (float*)R.rest(ws); }
    int32_t* sum(void* ws) const { return (int32_t*)((char*)R.rest(ws) + bias); }
    void* rest(void* ws) const { return (char*)R.rest(ws) + bias + sums; }
    size_t front() const { return R.lists + R.counts + bias + sums; }
};
bool soft_call_served(int n_feat, int n_pairs, int B, int H, int N, int D) {
    return region_call_served(n_feat, n_pairs, B, H, N, D) && (long)N * 255 < (1l << 31) && (long)n_feat * soft_stride(N) < (1l << 31);
}

// the lists over m != 0, then the biases and byte sums (also to sums_out, unless NULL)
int launch_soft_front(const SoftLayout& L, const PairArgs& a, const uint8_t* w, int n_feat, int32_t* sums_out, hipStream_t s) {
    int32_t *list = L.R.list(a.scratch), *cnt = L.R.cnt(a.scratch);
    const int st = launch_region_lists(w, n_feat, a.N, list, cnt, nullptr, s);
    if (st != DSIM_OK) return st;
    hipLaunchKernelGGL(soft_weights_kernel, dim3(n_feat), dim3(SOFT_THREADS), 0, s, bias_table(), w, a.N, soft_stride(a.N),
                       (const int32_t*)list, (const int32_t*)cnt, L.lb(a.scratch), L.sum(a.scratch), sums_out);
    DSIM_HIP_CHECK(hipGetLastError());
    return DSIM_OK;
}

template <typename T>
int launch_soft_maps_t(const PairArgs& a, const uint8_t* w, int n_feat, float* score, float* local, float* contrib, int32_t* status,
                       int32_t* sums, hipStream_t s) {
    const SoftLayout L(n_feat, a.N);
    int32_t *list = L.R.list(a.scratch), *cnt = L.R.cnt(a.scratch);
    float* part = (float*)L.rest(a.scratch);
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        int st = launch_soft_front(L, a, w, n_feat, sums, s);
        if (st != DSIM_OK) return st;
        st = launch_lds<soft_map_kernel<T, Dc>>(dim3((a.N + 127) / 128, a.B * a.H, a.n_pairs * 2), dim3(256), LDS, s, (const T*)a.q,
                                                (const T*)a.k, (const T*)a.v, (const int32_t*)list, (const int32_t*)cnt,
                                                (const float*)L.lb(a.scratch), w, soft_stride(a.N), a.idx_a, a.idx_b, a.B, a.H, a.N,
                                                scale_log2_of(Dc), a.similarity, part);
        if (st != DSIM_OK) return st;
        return launch_map_finish<RowsWeighted>(part, w, list, cnt, a, Dc, score, local, contrib, status, s);
    });
}

template <typename T>
int launch_soft_align_t(const PairArgs& a, const uint8_t* w, int n_feat, int grid_w, int32_t* match, float* weight, float* expect,
                        float* attn, int32_t* status, int32_t* sums, hipStream_t s) {
    const SoftLayout L(n_feat, a.N);
    int32_t *list = L.R.list(a.scratch), *cnt = L.R.cnt(a.scratch);
    float2* stats = (float2*)L.rest(a.scratch);
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value;
        const int qt = (a.N + 127) / 128, stride = soft_stride(a.N);
        const float c = scale_log2_of(Dc);
        const float* lb = L.lb(a.scratch);
        const int st = launch_soft_front(L, a, w, n_feat, sums, s);
        if (st != DSIM_OK) return st;
        if (attn) DSIM_HIP_CHECK(hipMemsetAsync(attn, 0, (size_t)a.n_pairs * 2 * a.N * a.N * sizeof(float), s));
        hipLaunchKernelGGL(region_align_off_kernel, dim3(a.n_pairs * 2), dim3(OFF_THREADS), 0, s, w, (const int32_t*)cnt, a.idx_a, a.idx_b,
                           a.N, match, weight, expect, status);
        DSIM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL((soft_align_stats_kernel<T, Dc>), dim3(qt, a.B * a.H, a.n_pairs * 2), dim3(256), 0, s, (const T*)a.q,
                           (const T*)a.k, (const int32_t*)list, (const int32_t*)cnt, lb, stride, a.idx_a, a.idx_b, a.B, a.H, a.N, c, stats);
        DSIM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL((soft_align_kernel<T, Dc>), dim3(qt, a.n_pairs * 2), dim3(256), 0, s, (const T*)a.q, (const T*)a.k,
                           (const int32_t*)list, (const int32_t*)cnt, lb, stride, a.idx_a, a.idx_b, a.B, a.H, a.N, c,
                           1.0f / (float)(a.B * a.H), grid_w, (const float2*)stats, match, weight, expect, attn, status);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
// 0 for a call launch_pair_score_maps_weights refuses for its shape
size_t pair_score_maps_weights_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    if (!soft_call_served(n_feat, n_pairs, B, H, N, D)) return 0;
    return SoftLayout(n_feat, N).front() + up256((size_t)n_pairs * 2 * 3 * B * H * N * sizeof(float));
}

// soft region maps: any head dim of DSIM_FOR_EACH_D, any N, the three dtypes
int launch_pair_score_maps_weights(const PairArgs& a, int dtype, const uint8_t* weights, int n_feat, float* score, float* local,
                                   float* contrib, int32_t* status, int32_t* weight_sums, hipStream_t s) {
    const int st = pair_args_check(a, dtype);
    if (st != DSIM_OK) return st;
    const size_t need = pair_score_maps_weights_scratch_bytes(n_feat, a.n_pairs, a.B, a.H, a.N, a.D);
    if (need == 0) return DSIM_ERR_INVALID;
    if (a.scratch_bytes < need) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype,
        [&](auto e) {
            return launch_soft_maps_t<typename decltype(e)::type>(a, weights, n_feat, score, local, contrib, status, weight_sums, s);
        },
        [&] { return DSIM_F16_TWIN(launch_pair_score_maps_weights(a, dtype, weights, n_feat, score, local, contrib, status, weight_sums, s)); });
}

// 0 for a call launch_pair_align_weights refuses for its shape
size_t pair_align_weights_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    if (!soft_call_served(n_feat, n_pairs, B, H, N, D)) return 0;
    return SoftLayout(n_feat, N).front() + up256((size_t)n_pairs * 2 * B * H * N * sizeof(float2));
}

// soft region alignments: any head dim of DSIM_FOR_EACH_D, any N, the three dtypes (a.v and a.similarity are not used)
int launch_pair_align_weights(const PairArgs& a, int dtype, const uint8_t* weights, int n_feat, int grid_w, int32_t* match, float* weight,
                              float* expect, float* attn, int32_t* status, int32_t* weight_sums, hipStream_t s) {
    const int st = pair_args_check(a, dtype);
    if (st != DSIM_OK) return st;
    if (grid_w < 1 || a.N % grid_w) return DSIM_ERR_INVALID;
    if (attn && (size_t)a.n_pairs * 2 * a.N * a.N * sizeof(float) >= ((size_t)1 << 31)) return DSIM_ERR_INVALID;
    const size_t need = pair_align_weights_scratch_bytes(n_feat, a.n_pairs, a.B, a.H, a.N, a.D);
    if (need == 0) return DSIM_ERR_INVALID;
    if (a.scratch_bytes < need) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype,
        [&](auto e) {
            return launch_soft_align_t<typename decltype(e)::type>(a, weights, n_feat, grid_w, match, weight, expect, attn, status,
                                                                  weight_sums, s);
        },
        [&] {
            return DSIM_F16_TWIN(launch_pair_align_weights(a, dtype, weights, n_feat, grid_w, match, weight, expect, attn, status, weight_sums, s));
        });
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
