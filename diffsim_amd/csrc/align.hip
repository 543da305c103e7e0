// Token alignments: the cross-attention the DiffSim score is built on, returned instead of consumed.  The score tail (tails.hip) is
// cross-attention of image A's queries over image B's keys -- diffsim/diffsim.py:177-180 of the reference -- and its fused kernels use
// softmax(Q_a K_b^T / sqrt(D)) in registers and drop it; these kernels compute that matrix for its own sake.  They share the tiled
// core's fragments, MFMA wrappers, K tile geometry and head-dim dispatch (attn_core.h), but not attend: there is no V and no O.
#include "align_core.h"

namespace dsim {
namespace {

// The two passes are align_core.h's bodies with the rows in order (the listed instantiations are region_maps.hip's).
// pass 1.  grid (ceil(N/128), B*H, n_pairs*2)
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void align_stats_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                             const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_b, int B,
                                                             int H, int N, float c, float2* __restrict__ stats) {
    align_stats_body<T, D, RowsInOrder>(qg, kg, nullptr, nullptr, idx_a, idx_b, B, H, N, c, stats);
}

// pass 2.  grid (ceil(N/128), n_pairs*2)
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void align_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                       const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_b, int B, int H,
                                                       int N, float c, float rbh, int grid_w, const float2* __restrict__ stats,
                                                       int32_t* __restrict__ match, float* __restrict__ weight, float* __restrict__ expect,
                                                       float* __restrict__ attn, int32_t* __restrict__ status) {
    align_body<T, D, RowsInOrder>(qg, kg, nullptr, nullptr, idx_a, idx_b, B, H, N, c, rbh, grid_w, stats, match, weight, expect, attn, status);
}

template <typename T>
int launch_align_t(const PairArgs& a, int grid_w, int32_t* match, float* weight, float* expect, float* attn, int32_t* status,
                   hipStream_t s) {
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value;
        const int qt = (a.N + 127) / 128;
        const float c = scale_log2_of(Dc);
        if (status) DSIM_HIP_CHECK(hipMemsetAsync(status, 0, (size_t)a.n_pairs * sizeof(int32_t), s));
        hipLaunchKernelGGL((align_stats_kernel<T, Dc>), dim3(qt, a.B * a.H, a.n_pairs * 2), dim3(256), 0, s, (const T*)a.q, (const T*)a.k,
                           a.idx_a, a.idx_b, a.B, a.H, a.N, c, (float2*)a.scratch);
        DSIM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL((align_kernel<T, Dc>), dim3(qt, a.n_pairs * 2), dim3(256), 0, s, (const T*)a.q, (const T*)a.k, a.idx_a, a.idx_b,
                           a.B, a.H, a.N, c, 1.0f / (float)(a.B * a.H), grid_w, (const float2*)a.scratch, match, weight, expect, attn,
                           status);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
// the statistics of align_stats_kernel, [pair][dir][bh][N] float2; 0 for a shape the launcher does not serve
size_t pair_align_scratch_bytes(int n_pairs, int B, int H, int N, int D) {
    if (!pair_shape_served(n_pairs, B, H, N, D)) return 0;
    return (size_t)n_pairs * 2 * B * H * N * sizeof(float2);
}

// token alignments (align_stats_kernel, align_kernel): any head dim of DSIM_FOR_EACH_D, any N, the three dtypes (a.v and
// a.similarity are not used)
int launch_pair_align(const PairArgs& a, int dtype, int grid_w, int32_t* match, float* weight, float* expect, float* attn,
                      int32_t* status, hipStream_t s) {
    const int st = pair_args_check(a, dtype);
    if (st != DSIM_OK) return st;
    if (grid_w < 1 || a.N % grid_w) return DSIM_ERR_INVALID;
    // 32-bit extents: an attention tensor stays below 2 GiB (the caller chunks the pairs); 16-byte aligned where its rows are
    // (N a multiple of 4: align_kernel stores four keys at a time)
    if (attn && ((size_t)a.n_pairs * 2 * a.N * a.N * sizeof(float) >= ((size_t)1 << 31) || ((a.N & 3) == 0 && ((uintptr_t)attn & 15))))
        return DSIM_ERR_INVALID;
    if (a.scratch_bytes < pair_align_scratch_bytes(a.n_pairs, a.B, a.H, a.N, a.D)) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype, [&](auto e) { return launch_align_t<typename decltype(e)::type>(a, grid_w, match, weight, expect, attn, status, s); },
        [&] { return DSIM_F16_TWIN(launch_pair_align(a, dtype, grid_w, match, weight, expect, attn, status, s)); });
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
