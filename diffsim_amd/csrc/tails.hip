// The fused DiffSim score tails on the tiled attention core (attn_core.h), for any shape and compute dtype; the default tap's
// persistent kernels are attn160.hip's.
//
//  * pair_tail_kernel: the DiffSim score tail -- /root/reference/diffsim/diffsim.py:177-197:
//                      O_ab = SDPA(Qa,Kb,Vb), O_aa = SDPA(Qa,Ka,Va) (and the b<->a mirror), then
//                      cosine (or mse) over the flattened (B,H,N,D) tensors.  Both attentions of a
//                      direction share Q and run in one workgroup; O never leaves registers, only
//                      three f32 partial sums per workgroup reach HBM and a second fixed-order pass
//                      folds them (no float atomics => bit-reproducible scores).
// pair_tail_kernel and pair_map_kernel name the in-order instantiations of tail_core.h's pair_tail_body (the listed one is
// regions.hip's); the score matrix launches the in-order instantiation of tail_core.h's matrix_tail_kernel (the listed one is
// region_matrix.hip's); the finish arithmetic, pair_finish_kernel, pair_map_finish_kernel and their launches are tail_core.h's too.  The launchers take PairArgs
// or MatrixArgs (common.h).
#include "tail_core.h"

namespace dsim {
namespace {

template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void pair_tail_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                        const T* __restrict__ vg, const int32_t* __restrict__ idx_a,
                                                        const int32_t* __restrict__ idx_b, int B, int H, int N,
                                                        float scale_log2, int mse, float* __restrict__ part) {
    pair_tail_body<T, D, false, RowsInOrder>(qg, kg, vg, nullptr, nullptr, idx_a, idx_b, B, H, N, scale_log2, mse, part);
}

template <typename T>
int launch_tail_t(const PairArgs& a, float* out, int32_t* status, hipStream_t s) {
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        const int qt = (a.N + 127) / 128;
        const int st = launch_lds<pair_tail_kernel<T, Dc>>(dim3(qt, a.B * a.H, a.n_pairs * 2), dim3(256), LDS, s, (const T*)a.q,
                                                           (const T*)a.k, (const T*)a.v, a.idx_a, a.idx_b, a.B, a.H, a.N,
                                                           scale_log2_of(Dc), a.similarity, (float*)a.scratch);
        if (st != DSIM_OK) return st;
        return launch_pair_finish<false>((const float*)a.scratch, nullptr, nullptr, nullptr, a.n_pairs, qt * a.B * a.H, a.similarity,
                                         (double)a.B * a.H * a.N * Dc, out, status, s);
    });
}

// score matrix: matrix_tail_kernel (tail_core.h) with the rows in order, the self mode once per image, then the cross mode once per
// cell and direction, and the pair finish over the cells
template <typename T>
int launch_matrix_t(const MatrixArgs& a, float* out, int32_t* status, hipStream_t s) {
    const MatrixLayout L(a, sizeof(T), false);
    const MatArgs m = L.kernel_args<MatArgs>(a);
    float* part = (float*)((char*)a.scratch + L.parts_at());
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        constexpr auto kernel = matrix_tail_kernel<T, Dc, RowsInOrder>;
        const int qt = (a.N + 127) / 128, nc = a.n_a * a.n_b, BH = a.B * a.H;
        int st = launch_lds<kernel>(dim3(qt, BH, a.n_a + a.n_b), dim3(256), LDS, s, m, scale_log2_of(Dc), a.similarity, 1, part);
        if (st != DSIM_OK) return st;
        st = launch_lds<kernel>(dim3(qt * nc * 2, BH), dim3(256), LDS, s, m, scale_log2_of(Dc), a.similarity, 0, part);
        if (st != DSIM_OK) return st;
        return launch_pair_finish<false>(part, nullptr, nullptr, nullptr, nc, qt * BH, a.similarity, (double)BH * a.N * Dc, out, status, s);
    });
}

// ---- similarity maps: the score tail kept per token ------------------------------------------------------------------------------
// The score of direction a->b splits over query tokens: cos(O_ab, O_aa) = sum_i dot_i / (|O_ab| |O_aa|) and
// mse = sum_i sqd_i / (B H N D), where dot_i / sqd_i sum over the CFG batch, the heads and d at token i.
// pair_map_kernel is pair_tail_body with the per-token epilogue: pair_tail_kernel's grid, attentions, rounding and products, so that
// a pair's map contributions sum to its score; the finish is tail_core.h's pair_map_finish_kernel with the rows in order.
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void pair_map_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                        const T* __restrict__ vg, const int32_t* __restrict__ idx_a,
                                                        const int32_t* __restrict__ idx_b, int B, int H, int N,
                                                        float scale_log2, int mse, float* __restrict__ part) {
    pair_tail_body<T, D, true, RowsInOrder>(qg, kg, vg, nullptr, nullptr, idx_a, idx_b, B, H, N, scale_log2, mse, part);
}

template <typename T>
int launch_maps_t(const PairArgs& a, float* score, float* local, float* contrib, int32_t* status, hipStream_t s) {
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        const int st = launch_lds<pair_map_kernel<T, Dc>>(dim3((a.N + 127) / 128, a.B * a.H, a.n_pairs * 2), dim3(256), LDS, s,
                                                          (const T*)a.q, (const T*)a.k, (const T*)a.v, a.idx_a, a.idx_b, a.B, a.H, a.N,
                                                          scale_log2_of(Dc), a.similarity, (float*)a.scratch);
        if (st != DSIM_OK) return st;
        return launch_map_finish<RowsInOrder>((const float*)a.scratch, nullptr, nullptr, nullptr, a, Dc, score, local, contrib, status, s);
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
// The shapes a pair launcher serves: at least one pair, image and token; two directions per pair on a 65535-wide grid axis and, for
// the tiled kernels, B*H on another; a head dim of DSIM_FOR_EACH_D
bool pair_shape_served(int n_pairs, int B, int H, int N, int D, bool tiled) {
    if (n_pairs < 1 || B < 1 || H < 1 || N < 1) return false;
    if (n_pairs > 65535 / 2 || (tiled && (long)B * H > 65535)) return false;
    return with_head_dim(D, [](auto) { return DSIM_OK; }) == DSIM_OK;
}

size_t pair_score_scratch_bytes(int n_pairs, int B, int H, int N, int D) {
    const size_t tiled = (size_t)n_pairs * 2 * B * H * ((N + 127) / 128) * 4 * sizeof(float);
    if (pair_score160_applies(N, D, DSIM_H16)) {          // (dtype-blind: the 16-bit modes' persistent kernel needs the larger workspace)
        const size_t pers = pair_score160_scratch_bytes(n_pairs, B, H);
        return pers > tiled ? pers : tiled;
    }
    return tiled;
}

// the default tap in a 16-bit mode runs the persistent kernel (attn160.hip), whose grid carries B*H on no axis
int launch_pair_score(const PairArgs& a, int dtype, float* out, int32_t* status, hipStream_t s) {
    const bool p160 = dtype != DSIM_F32 && pair_score160_applies(a.N, a.D, DSIM_H16);
    const int st = pair_args_check(a, dtype, !p160);
    if (st != DSIM_OK) return st;
    if (a.scratch_bytes < pair_score_scratch_bytes(a.n_pairs, a.B, a.H, a.N, a.D)) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype,
        [&](auto e) {
            typedef typename decltype(e)::type T;
            if constexpr (sizeof(T) == 2)
                if (p160) return launch_pair_score160(a, out, status, s);
            return launch_tail_t<T>(a, out, status, s);
        },
        [&] { return DSIM_F16_TWIN(launch_pair_score(a, dtype, out, status, s)); });
}

// The matrix calls served, for both launchers, both workspace queries and both entry points: a dtype of the three, a head dim of
// DSIM_FOR_EACH_D, at least one image per set, one token, one head; n_a + n_b on the self grid's 65535-wide axis and the cross grid in
// a 32-bit extent.  Then what the kernels of the call index in 32 bits: the persistent default-tap kernels (16-bit, unmasked) their
// per-wave partial slots and the bytes of a (batch element, head) view; the tiled kernels B*H on a 65535-wide grid axis (their
// offsets are 64-bit), the unmasked call keeping the persistent one's bound on the partial slots; the listed call every tensor and
// list under 2^31 elements.
bool matrix_shape_served(int n_a, int n_b, int B, int H, int N, int D, int dtype, bool listed) {
    if (dtype != DSIM_F32 && dtype != DSIM_BF16 && dtype != DSIM_F16) return false;
    if (n_a < 1 || n_b < 1 || B < 1 || H < 1 || N < 1) return false;
    if (with_head_dim(D, [](auto) { return DSIM_OK; }) != DSIM_OK) return false;
    const long lim = 1l << 31, qt = (N + 127) / 128, nc = (long)n_a * n_b, bh = (long)B * H;
    if ((long)n_a + n_b > 65535 || nc * 2 * qt >= lim) return false;
    // the unmasked call's partial slots (bh < 2^27 first, so that the product cannot overflow)
    const bool slots_ok = bh < lim / 16 && nc * bh * 16 < lim;
    if (listed) {                                                                 // the tiled kernel over listed rows
        if (bh > 65535) return false;
        const long row = bh * D, mx = n_a > n_b ? n_a : n_b;                      // (row < 2^16 * 2^8)
        if (row >= lim / N || row * N >= lim / mx) return false;                  // a set's q, k, v and self output
        if (((long)n_a + n_b) * N >= lim) return false;                           // the lists
        return nc * 2 * qt < lim / (bh * 4);                                      // the partials
    } else if (dtype != DSIM_F32 && pair_score160_applies(N, D, DSIM_H16)) {      // the persistent default-tap kernels
        return slots_ok && (long)(N - 1) * H * D * 2 + D * 2 < lim;               // a view's last row, in bytes
    } else {                                                                      // the tiled kernel, rows in order
        return bh <= 65535 && slots_ok;
    }
}

size_t score_matrix_scratch_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    if (!matrix_shape_served(n_a, n_b, B, H, N, D, dtype, false)) return 0;
    if (dtype != DSIM_F32 && pair_score160_applies(N, D, DSIM_H16))
        return score_matrix160_scratch_bytes(n_a, n_b, B, H);           // (the fp16 persistent kernel has the bf16 one's layout)
    return MatrixLayout({{}, {}, {}, {}, n_a, n_b, B, H, N, D}, dtype_size(dtype), false).total();
}

// the default tap in a 16-bit mode runs the persistent kernels (attn160.hip)
int launch_score_matrix(const MatrixArgs& a, int dtype, float* out, int32_t* status, hipStream_t s) {
    const int st = matrix_args_check(a, dtype, false);
    if (st != DSIM_OK) return st;
    if (a.scratch_bytes < score_matrix_scratch_bytes(a.n_a, a.n_b, a.B, a.H, a.N, a.D, dtype)) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype,
        [&](auto e) {
            typedef typename decltype(e)::type T;
            if constexpr (sizeof(T) == 2)
                if (pair_score160_applies(a.N, a.D, DSIM_H16)) return launch_score_matrix160(a, out, status, s);
            return launch_matrix_t<T>(a, out, status, s);
        },
        [&] { return DSIM_F16_TWIN(launch_score_matrix(a, dtype, out, status, s)); });
}

size_t pair_score_maps_scratch_bytes(int n_pairs, int B, int H, int N) {
    if (n_pairs < 1 || B < 1 || H < 1 || N < 1) return 0;
    return (size_t)n_pairs * 2 * 3 * B * H * N * sizeof(float);
}

// per-token maps of the score tail: pair_map_kernel at every shape and dtype (the default tap's persistent kernel keeps no
// per-token sums)
int launch_pair_score_maps(const PairArgs& a, int dtype, float* score, float* local, float* contrib, int32_t* status, hipStream_t s) {
    const int st = pair_args_check(a, dtype);
    if (st != DSIM_OK) return st;
    if (a.scratch_bytes < pair_score_maps_scratch_bytes(a.n_pairs, a.B, a.H, a.N)) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype, [&](auto e) { return launch_maps_t<typename decltype(e)::type>(a, score, local, contrib, status, s); },
        [&] { return DSIM_F16_TWIN(launch_pair_score_maps(a, dtype, score, local, contrib, status, s)); });
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
