// Soft region scores: the region score (regions.hip) with a weight per token instead of an on/off bit.  Every feature image i carries
// a byte m_i[t] in 0 .. 255 per token, w = m / 255.  A token of weight 0 is dropped as the region score drops an off token; a token
// of weight w takes part in every softmax as a key with the additive logit bias ln w, and as a query with the factor w on its terms
// of the cosine / mse sums (include/diffsim_amd.h, dsim_pair_score_weights).  Weights are multiplicities: a token of byte 2c is two
// identical tokens of byte c.
//
//   the lists             regions.hip's region_lists_kernel over m != 0 (launch_region_lists, the one source of it)
//   soft_weights_kernel   (soft_core.h) per image: the listed tokens' biases log2(m / 255) by compacted position -- from a 256-entry f32 table the host
//                         builds in double and rounds once (entry 255 is 0.0f, entry 1 about -7.99), padded with zeros to whole
//                         64-key tiles -- and the image's byte sum
//   soft_tail_kernel      pair_tail_body (tail_core.h) with RowsWeighted: the region tail's program text, attend with KeyBiasLog2 in
//                         both attentions (each with the key image's biases), the lane's three sums times the query row's byte / 255
//   soft_finish_kernel    (soft_core.h) pair_finish_kernel's fold; the mse count of a direction is B H D (byte sum of the query image) / 255 in f64;
//                         an image of byte sum 0: NaN, status 2
// With every byte 0 or 255 each addition is + 0.0f and each factor 1.0f, and (255 n) / 255 is n: the region score's bits.
//
// Where the biases live: in global memory, read per tile -- 64 floats a tile, eight 16-byte loads per lane (attn_core.h, attend).
// They are not staged in LDS.  ACfg<T, D>::LDS is what this tail asks for, as the region tail does, per (T, D): 16-bit d = 16: 14 KB,
// 32: 18 KB, 40: 38 KB, 64: 42 KB, 72 / 80: 46 KB (two K / V tile pairs each), 160: 41 KB (one pair); f32 (one pair): d = 16 / 32: 18 KB,
// 40 / 64: 34 KB, 72 / 80: 50 KB, 160: 82 KB.  The workgroups a CU holds are set by the registers except where LDS binds first: the
// 16-bit d = 40 tail (164 registers: three waves a SIMD, three workgroups of 38 KB in the CU's 160 KB) is the 4096-token tap of SD1.5,
// and a 16 KB bias array for N = 4096 beside its tiles (54 KB) would leave it two.  So no (T, D) stages the biases.
// In its own translation unit for regions.hip's reason: one more instantiation of attend per head dim and dtype that cannot move the
// code of the others.
#include "soft_core.h"

namespace dsim {
namespace {

// One direction of a pair in a workgroup of 128 compacted query positions: pair_tail_body with weighted listed rows.
// grid (ceil(N/128), B*H, n_pairs*2), the region tail's.  part: [pair][dir][bh][qtile][4] f32
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void soft_tail_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                        const T* __restrict__ vg, const int32_t* __restrict__ list,
                                                        const int32_t* __restrict__ cnt, const float* __restrict__ lb,
                                                        const uint8_t* __restrict__ w, int stride, const int32_t* __restrict__ idx_a,
                                                        const int32_t* __restrict__ idx_b, int B, int H, int N,
                                                        float scale_log2, int mse, float* __restrict__ part) {
    pair_tail_body<T, D, false, RowsWeighted>(qg, kg, vg, list, cnt, idx_a, idx_b, B, H, N, scale_log2, mse, part,
                                              RowsWeighted::Table{lb, w, stride});
}

// workspace: [lists int32 [n_feat][N] | counts int32 [n_feat] | biases f32 [n_feat][stride] | byte sums int32 [n_feat] |
//             partials f32 [n_pairs][2][B H][qtiles][4]], each 256-byte aligned (the sizes: soft_core.h)
template <typename T>
int launch_weights_t(const PairArgs& a, const uint8_t* w, int n_feat, float* out, int32_t* status, int32_t* sums, hipStream_t s) {
    int32_t* list = (int32_t*)a.scratch;
    int32_t* cnt = (int32_t*)((char*)list + soft_list_bytes(n_feat, a.N));
    float* lb = (float*)((char*)cnt + soft_count_bytes(n_feat));
    int32_t* sum = (int32_t*)((char*)lb + soft_bias_bytes(n_feat, a.N));
    float* part = (float*)((char*)sum + soft_count_bytes(n_feat));
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        const int qt = (a.N + 127) / 128, stride = soft_stride(a.N);
        int st = launch_region_lists(w, n_feat, a.N, list, cnt, nullptr, s);
        if (st != DSIM_OK) return st;
        hipLaunchKernelGGL(soft_weights_kernel, dim3(n_feat), dim3(SOFT_THREADS), 0, s, bias_table(), w, a.N, stride, (const int32_t*)list,
                           (const int32_t*)cnt, lb, sum, sums);
        DSIM_HIP_CHECK(hipGetLastError());
        st = launch_lds<soft_tail_kernel<T, Dc>>(dim3(qt, a.B * a.H, a.n_pairs * 2), dim3(256), LDS, s, (const T*)a.q, (const T*)a.k,
                                                 (const T*)a.v, (const int32_t*)list, (const int32_t*)cnt, (const float*)lb, w, stride,
                                                 a.idx_a, a.idx_b, a.B, a.H, a.N, scale_log2_of(Dc), a.similarity, part);
        if (st != DSIM_OK) return st;
        hipLaunchKernelGGL(soft_finish_kernel, dim3((a.n_pairs + 63) / 64), dim3(64), 0, s, (const float*)part, (const int32_t*)sum, a.idx_a,
                           a.idx_b, a.n_pairs, qt * a.B * a.H, a.similarity, (double)a.B * a.H * Dc, out, status);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
// 0 for a call launch_pair_score_weights refuses for its shape: the region score's refusals, and a byte sum that could pass int32
size_t pair_score_weights_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    if (n_feat < 1 || !pair_shape_served(n_pairs, B, H, N, D) || (long)n_feat * soft_stride(N) >= (1l << 31) || (long)N * 255 >= (1l << 31))
        return 0;
    return soft_list_bytes(n_feat, N) + 2 * soft_count_bytes(n_feat) + soft_bias_bytes(n_feat, N) +
           up256((size_t)n_pairs * 2 * B * H * ((N + 127) / 128) * 4 * sizeof(float));
}

// soft region scores (region_lists_kernel, soft_weights_kernel, soft_tail_kernel, soft_finish_kernel): any head dim of
// DSIM_FOR_EACH_D, any N, the three dtypes
int launch_pair_score_weights(const PairArgs& a, int dtype, const uint8_t* weights, int n_feat, float* out, int32_t* status,
                              int32_t* weight_sums, hipStream_t s) {
    const int st = pair_args_check(a, dtype);
    if (st != DSIM_OK) return st;
    const size_t need = pair_score_weights_scratch_bytes(n_feat, a.n_pairs, a.B, a.H, a.N, a.D);
    if (need == 0) return DSIM_ERR_INVALID;
    if (a.scratch_bytes < need) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype, [&](auto e) { return launch_weights_t<typename decltype(e)::type>(a, weights, n_feat, out, status, weight_sums, s); },
        [&] { return DSIM_F16_TWIN(launch_pair_score_weights(a, dtype, weights, n_feat, out, status, weight_sums, s)); });
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
