// Region maps and region alignments: the per-token outputs of the score tail and of the cross-attention, restricted to a token region
// per image.  Every feature image i carries a region R_i of its N tokens (a byte mask, non-zero = on; regions.hip); its on tokens
// ascending are list[i][0 .. cnt[i]), compacted position t is row list[i][t], and cnt[i] stands wherever N stood.  The off tokens are
// neither queries nor keys.  The outputs lie on the full token grid.
//
//   region_map_kernel        pair_map_kernel's arithmetic -- tail_core.h's pair_tail_body with the per-token epilogue -- with the rows
//                            taken through the lists (RowsListed): the region tail's own attentions, rounding and products, kept per
//                            query position.  Partials [pair][dir][comp][bh][N] by position; a workgroup past the query image's
//                            count, or of a pair with an empty image, leaves before any barrier and writes nothing
//   the map finish           pair_map_finish_kernel<RowsListed> (tail_core.h): the in-order finish's folds over t < cnt, scattered to
//                            token list[t]; zeros at the off tokens; an empty region reported (NaN, status 2, zero maps)
//   region_align_off_kernel  (region_maps_core.h) the off values of the alignments (match -1, weight 0, expect (-1, -1)) at every off query token and on
//                            every row of a pair with an empty image, and the status word of each pair (0, or 2 for an empty image)
//   region_align_stats_kernel / region_align_kernel
//                            align_core.h's two passes with listed rows: keys gathered through the key image's list, queries through
//                            the query image's, coordinates and match on the full grid, outputs scattered to the query's token
// With every region full the outputs are dsim_pair_score_maps' and dsim_pair_align's bits.
// The kernels are instantiated here, not in tails.hip or align.hip, for regions.hip's reason: in a translation unit of their own they
// cannot move the register allocation or the code of the existing tails.
#include "region_maps_core.h"

namespace dsim {
namespace {

// One direction of a pair in a workgroup of 128 compacted query positions: pair_tail_body, per token, with listed rows.
// grid (ceil(N/128), B*H, n_pairs*2): the worst case, the counts being on the device.  part: [pair][dir][comp][bh][N] f32
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void region_map_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                        const T* __restrict__ vg, const int32_t* __restrict__ list,
                                                        const int32_t* __restrict__ cnt, const int32_t* __restrict__ idx_a,
                                                        const int32_t* __restrict__ idx_b, int B, int H, int N,
                                                        float scale_log2, int mse, float* __restrict__ part) {
    pair_tail_body<T, D, true, RowsListed>(qg, kg, vg, list, cnt, idx_a, idx_b, B, H, N, scale_log2, mse, part);
}

// pass 1 of the alignments over listed rows.  grid (ceil(N/128), B*H, n_pairs*2); stats [pair][dir][bh][N] float2 by position
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void region_align_stats_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                             const int32_t* __restrict__ list, const int32_t* __restrict__ cnt,
                                                             const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_b, int B,
                                                             int H, int N, float c, float2* __restrict__ stats) {
    align_stats_body<T, D, RowsListed>(qg, kg, list, cnt, idx_a, idx_b, B, H, N, c, stats);
}

// pass 2.  grid (ceil(N/128), n_pairs*2)
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void region_align_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                       const int32_t* __restrict__ list, const int32_t* __restrict__ cnt,
                                                       const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_b, int B, int H,
                                                       int N, float c, float rbh, int grid_w, const float2* __restrict__ stats,
                                                       int32_t* __restrict__ match, float* __restrict__ weight, float* __restrict__ expect,
                                                       float* __restrict__ attn, int32_t* __restrict__ status) {
    align_body<T, D, RowsListed>(qg, kg, list, cnt, idx_a, idx_b, B, H, N, c, rbh, grid_w, stats, match, weight, expect, attn, status);
}

template <typename T>
int launch_region_maps_t(const PairArgs& a, const uint8_t* mask, int n_feat, float* score, float* local, float* contrib, int32_t* status,
                         int32_t* counts, hipStream_t s) {
    const RegionLayout L(n_feat, a.N);
    int32_t *list = L.list(a.scratch), *cnt = L.cnt(a.scratch);
    float* part = (float*)L.rest(a.scratch);
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        int st = launch_region_lists(mask, n_feat, a.N, list, cnt, counts, s);
        if (st != DSIM_OK) return st;
        st = launch_lds<region_map_kernel<T, Dc>>(dim3((a.N + 127) / 128, a.B * a.H, a.n_pairs * 2), dim3(256), LDS, s, (const T*)a.q,
                                                  (const T*)a.k, (const T*)a.v, (const int32_t*)list, (const int32_t*)cnt, a.idx_a, a.idx_b,
                                                  a.B, a.H, a.N, scale_log2_of(Dc), a.similarity, part);
        if (st != DSIM_OK) return st;
        return launch_map_finish<RowsListed>(part, mask, list, cnt, a, Dc, score, local, contrib, status, s);
    });
}

template <typename T>
int launch_region_align_t(const PairArgs& a, const uint8_t* mask, int n_feat, int grid_w, int32_t* match, float* weight, float* expect,
                          float* attn, int32_t* status, int32_t* counts, hipStream_t s) {
    const RegionLayout L(n_feat, a.N);
    int32_t *list = L.list(a.scratch), *cnt = L.cnt(a.scratch);
    float2* stats = (float2*)L.rest(a.scratch);
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value;
        const int qt = (a.N + 127) / 128;
        const float c = scale_log2_of(Dc);
        const int st = launch_region_lists(mask, n_feat, a.N, list, cnt, counts, s);
        if (st != DSIM_OK) return st;
        if (attn) DSIM_HIP_CHECK(hipMemsetAsync(attn, 0, (size_t)a.n_pairs * 2 * a.N * a.N * sizeof(float), s));
        hipLaunchKernelGGL(region_align_off_kernel, dim3(a.n_pairs * 2), dim3(OFF_THREADS), 0, s, mask, (const int32_t*)cnt, a.idx_a, a.idx_b,
                           a.N, match, weight, expect, status);
        DSIM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL((region_align_stats_kernel<T, Dc>), dim3(qt, a.B * a.H, a.n_pairs * 2), dim3(256), 0, s, (const T*)a.q,
                           (const T*)a.k, (const int32_t*)list, (const int32_t*)cnt, a.idx_a, a.idx_b, a.B, a.H, a.N, c, stats);
        DSIM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL((region_align_kernel<T, Dc>), dim3(qt, a.n_pairs * 2), dim3(256), 0, s, (const T*)a.q, (const T*)a.k,
                           (const int32_t*)list, (const int32_t*)cnt, a.idx_a, a.idx_b, a.B, a.H, a.N, c, 1.0f / (float)(a.B * a.H), grid_w,
                           (const float2*)stats, match, weight, expect, attn, status);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
// 0 for a call launch_pair_score_maps_regions refuses for its shape
size_t pair_score_maps_regions_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    if (!region_call_served(n_feat, n_pairs, B, H, N, D)) return 0;
    const RegionLayout L(n_feat, N);
    return L.lists + L.counts + up256((size_t)n_pairs * 2 * 3 * B * H * N * sizeof(float));
}

// region maps (region_lists_kernel, region_map_kernel, pair_map_finish_kernel<RowsListed>): any head dim of DSIM_FOR_EACH_D, any N,
// the three dtypes
int launch_pair_score_maps_regions(const PairArgs& a, int dtype, const uint8_t* mask, int n_feat, float* score, float* local,
                                   float* contrib, int32_t* status, int32_t* counts, hipStream_t s) {
    const int st = pair_args_check(a, dtype);
    if (st != DSIM_OK) return st;
    const size_t need = pair_score_maps_regions_scratch_bytes(n_feat, a.n_pairs, a.B, a.H, a.N, a.D);
    if (need == 0) return DSIM_ERR_INVALID;
    if (a.scratch_bytes < need) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype,
        [&](auto e) { return launch_region_maps_t<typename decltype(e)::type>(a, mask, n_feat, score, local, contrib, status, counts, s); },
        [&] { return DSIM_F16_TWIN(launch_pair_score_maps_regions(a, dtype, mask, n_feat, score, local, contrib, status, counts, s)); });
}

// 0 for a call launch_pair_align_regions refuses for its shape
size_t pair_align_regions_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    if (!region_call_served(n_feat, n_pairs, B, H, N, D)) return 0;
    const RegionLayout L(n_feat, N);
    return L.lists + L.counts + up256((size_t)n_pairs * 2 * B * H * N * sizeof(float2));
}

// region alignments (region_lists_kernel, region_align_off_kernel, region_align_stats_kernel, region_align_kernel): any head dim of
// DSIM_FOR_EACH_D, any N, the three dtypes (a.v and a.similarity are not used)
int launch_pair_align_regions(const PairArgs& a, int dtype, const uint8_t* mask, int n_feat, int grid_w, int32_t* match, float* weight,
                              float* expect, float* attn, int32_t* status, int32_t* counts, hipStream_t s) {
    const int st = pair_args_check(a, dtype);
    if (st != DSIM_OK) return st;
    if (grid_w < 1 || a.N % grid_w) return DSIM_ERR_INVALID;
    // 32-bit extents: an attention tensor stays below 2 GiB (the caller chunks the pairs)
    if (attn && (size_t)a.n_pairs * 2 * a.N * a.N * sizeof(float) >= ((size_t)1 << 31)) return DSIM_ERR_INVALID;
    const size_t need = pair_align_regions_scratch_bytes(n_feat, a.n_pairs, a.B, a.H, a.N, a.D);
    if (need == 0) return DSIM_ERR_INVALID;
    if (a.scratch_bytes < need) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype,
        [&](auto e) {
            return launch_region_align_t<typename decltype(e)::type>(a, mask, n_feat, grid_w, match, weight, expect, attn, status, counts, s);
        },
        [&] { return DSIM_F16_TWIN(launch_pair_align_regions(a, dtype, mask, n_feat, grid_w, match, weight, expect, attn, status, counts, s)); });
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
