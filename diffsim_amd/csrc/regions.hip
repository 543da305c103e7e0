// Region scores: the DiffSim score tail restricted to a token region per image.  Every feature image i carries a region
// R_i of its N tokens (a byte mask, non-zero = on); the region score of (a, b) is the reference's tail -- diffsim/diffsim.py:177-197 --
// on the sub-tensors Q_a[R_a], K_a[R_a], V_a[R_a] and Q_b[R_b], K_b[R_b], V_b[R_b], rows in ascending token order: the off tokens are
// neither queries nor keys, so they take part in no softmax.  With every region full it is the pair score.
//
//   region_lists_kernel   the masks as ascending token lists and counts (the workspace)
//   region_tail_kernel    pair_tail_kernel's arithmetic -- the same source text, tail_core.h's pair_tail_body: attend twice on one
//                         set of Q fragments, the rounding, the products, the partial layout -- with the rows taken through the
//                         lists (RowsListed): compacted position t of an image is its row list[t], and the image's count stands
//                         where N stood
//   the finish            pair_finish_kernel<true> (tail_core.h): the pair tail's fixed-order f64 fold, the direction's own element
//                         count for mse, and an empty region reported instead of scored
// The region tail is instantiated here, not in tails.hip: it is one more instantiation of attend per head dim and dtype, and in its
// own translation unit it cannot move the register allocation or the code of the pair, map and matrix tails.
#include "tail_core.h"

namespace dsim {
namespace {

constexpr int LIST_THREADS = 256;

// One workgroup per feature image: list[img][0 .. count) = the on tokens ascending, cnt[img] = count (also to counts_out when the
// caller asked).  256 tokens a round: a ballot per wave, the lane's rank from the lower lanes' bits, the waves' totals through LDS.
// Every entry has one writer; the entries from count on are not written and never read.
__global__ __launch_bounds__(LIST_THREADS) void region_lists_kernel(const uint8_t* __restrict__ mask, int N, int32_t* __restrict__ list,
                                                                    int32_t* __restrict__ cnt, int32_t* __restrict__ counts_out) {
    __shared__ int wtot[LIST_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* m = mask + (size_t)blockIdx.x * N;
    int32_t* out = list + (size_t)blockIdx.x * N;
    int base = 0;
    for (int t0 = 0; t0 < N; t0 += LIST_THREADS) {
        const int t = t0 + tid;
        const bool on = t < N && m[t] != 0;
        const unsigned long long bits = __ballot(on);
        const int rank = __popcll(bits & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wave] = __popcll(bits);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < LIST_THREADS / 64; ++w) {
            if (w < wave) before += wtot[w];
            total += wtot[w];
        }
        if (on) out[base + before + rank] = t;
        base += total;
        __syncthreads();                   // (wtot is read before the next round writes it)
    }
    if (tid == 0) {
        cnt[blockIdx.x] = base;
        if (counts_out) counts_out[blockIdx.x] = base;
    }
}

// One direction of a pair in a workgroup of 128 compacted query positions: pair_tail_body with listed rows.
// grid (ceil(N/128), B*H, n_pairs*2): the worst case, the counts being on the device.  part: [pair][dir][bh][qtile][4] f32
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void region_tail_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                        const T* __restrict__ vg, const int32_t* __restrict__ list,
                                                        const int32_t* __restrict__ cnt, const int32_t* __restrict__ idx_a,
                                                        const int32_t* __restrict__ idx_b, int B, int H, int N,
                                                        float scale_log2, int mse, float* __restrict__ part) {
    pair_tail_body<T, D, false, RowsListed>(qg, kg, vg, list, cnt, idx_a, idx_b, B, H, N, scale_log2, mse, part);
}

// workspace: [lists int32 [n_feat][N] | counts int32 [n_feat] | partials f32 [n_pairs][2][B H][qtiles][4]], each 256-byte aligned
size_t region_list_bytes(int n_feat, int N) { return up256((size_t)n_feat * N * sizeof(int32_t)); }
size_t region_count_bytes(int n_feat) { return up256((size_t)n_feat * sizeof(int32_t)); }

template <typename T>
int launch_regions_t(const PairArgs& a, const uint8_t* mask, int n_feat, float* out, int32_t* status, int32_t* counts, hipStream_t s) {
    int32_t* list = (int32_t*)a.scratch;
    int32_t* cnt = (int32_t*)((char*)a.scratch + region_list_bytes(n_feat, a.N));
    float* part = (float*)((char*)cnt + region_count_bytes(n_feat));
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        const int qt = (a.N + 127) / 128;
        int st = launch_region_lists(mask, n_feat, a.N, list, cnt, counts, s);
        if (st != DSIM_OK) return st;
        st = launch_lds<region_tail_kernel<T, Dc>>(dim3(qt, a.B * a.H, a.n_pairs * 2), dim3(256), LDS, s, (const T*)a.q,
                                                             (const T*)a.k, (const T*)a.v, (const int32_t*)list, (const int32_t*)cnt,
                                                             a.idx_a, a.idx_b, a.B, a.H, a.N, scale_log2_of(Dc), a.similarity, part);
        if (st != DSIM_OK) return st;
        return launch_pair_finish<true>(part, cnt, a.idx_a, a.idx_b, a.n_pairs, qt * a.B * a.H, a.similarity, (double)a.B * a.H * Dc, out, status, s);
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
// region_lists_kernel over n_feat masks: the one launch site, for the region tail here and the region matrix (region_matrix.hip)
int launch_region_lists(const uint8_t* mask, int n_feat, int N, int32_t* list, int32_t* cnt, int32_t* counts, hipStream_t s) {
    hipLaunchKernelGGL(region_lists_kernel, dim3(n_feat), dim3(LIST_THREADS), 0, s, mask, N, list, cnt, counts);
    DSIM_HIP_CHECK(hipGetLastError());
    return DSIM_OK;
}

// 0 for a call launch_pair_score_regions refuses for its shape
size_t pair_score_regions_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    if (n_feat < 1 || !pair_shape_served(n_pairs, B, H, N, D) || (long)n_feat * N >= (1l << 31)) return 0;
    return region_list_bytes(n_feat, N) + region_count_bytes(n_feat) + up256((size_t)n_pairs * 2 * B * H * ((N + 127) / 128) * 4 * sizeof(float));
}

// region scores (region_lists_kernel, region_tail_kernel, pair_finish_kernel<true>): any head dim of DSIM_FOR_EACH_D, any N, the
// three dtypes; the default tap runs the tiled kernel too
int launch_pair_score_regions(const PairArgs& a, int dtype, const uint8_t* mask, int n_feat, float* out, int32_t* status,
                              int32_t* counts, hipStream_t s) {
    const int st = pair_args_check(a, dtype);
    if (st != DSIM_OK) return st;
    const size_t need = pair_score_regions_scratch_bytes(n_feat, a.n_pairs, a.B, a.H, a.N, a.D);
    if (need == 0) return DSIM_ERR_INVALID;
    if (a.scratch_bytes < need) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype, [&](auto e) { return launch_regions_t<typename decltype(e)::type>(a, mask, n_feat, out, status, counts, s); },
        [&] { return DSIM_F16_TWIN(launch_pair_score_regions(a, dtype, mask, n_feat, out, status, counts, s)); });
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
