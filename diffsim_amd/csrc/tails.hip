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
// regions.hip's); the finish arithmetic and pair_finish_kernel are tail_core.h's too.  The launchers take PairArgs (common.h).
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

// ---- score matrix ---------------------------------------------------------------------------------------------------------------
// Every image of set A against every image of set B.  The score of (a, b) needs O_aa and O_bb, which do not depend on the partner: the
// SELF mode computes each image's once (rounded to the compute dtype as the pair tail rounds it; f32 in the parity mode) into
// [n][B][N][H*D], and the CROSS mode runs one attention per cell and direction -- O_ab = SDPA(Qa, Kb, Vb) against O_aa read back,
// O_ba = SDPA(Qb, Ka, Va) against O_bb -- with the pair tail's products, reduction and partial layout [cell][dir][bh][qtile][4], so
// pair_finish_kernel folds them.  Both modes run the same attend on the same Q fragments as pair_tail_kernel: a cell of an image
// against itself compares bit-identical tensors, and a cell equals the pair tail's score of the same two images.
// grid  self: (ceil(N/128), B*H, n_a + n_b);  cross: (ceil(N/128) * n_cells * 2, B*H)
struct MatArgs {
    const void* q[2]; const void* k[2]; const void* v[2];      // set A, set B: [n][B][N][H*D]
    void* self[2];                                              // the sets' self outputs, same layout
    int n_a, n_b, B, H, N;
};
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void matrix_tail_kernel(const MatArgs p, float scale_log2, int mse, int self_mode,
                                                                                     float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
    const int N = p.N, ld = p.H * D;
    const size_t img = (size_t)p.B * N * ld;
    const size_t boff = (size_t)b * N * ld + h * D;
    const int qt = (N + 127) / 128;
    int qtile, set, iq, ix, cell = 0, dir = 0;
    if (self_mode) {
        qtile = blockIdx.x;
        set = (int)blockIdx.z >= p.n_a;
        iq = ix = (int)blockIdx.z - (set ? p.n_a : 0);
    } else {
        qtile = blockIdx.x % qt;
        const int cd = blockIdx.x / qt;
        cell = cd >> 1; dir = cd & 1;
        const int ia = cell / p.n_b, ib = cell - ia * p.n_b;
        set = dir;
        iq = dir ? ib : ia;
        ix = dir ? ia : ib;
    }
    const T* qg = (const T*)p.q[set];
    const T* kg = (const T*)p.k[set ^ (self_mode ? 0 : 1)];
    const T* vg = (const T*)p.v[set ^ (self_mode ? 0 : 1)];
    T* so = (T*)p.self[set] + iq * img + boff;
    const int q = qtile * 128 + wave * 32 + l31;
    const int qc = q < N ? q : N - 1;
    QFrags<T, D> qf;
    load_q<T, D>(qf, qg + iq * img + boff + (size_t)qc * ld, half, scale_log2);
    OAcc<T, D> oa;
    attend<T, D>(qf, kg + ix * img + boff, vg + ix * img + boff, ld, N, smem, oa);
    settle<T, D>(oa);
    if (self_mode) {
        if (q < N) fold_rounded<T, D>(oa, half, 0, [&](int, int, int, int d, T y) { so[(size_t)q * ld + d] = y; return 0; });  // (no state)
        return;
    }
    TailSums t;
    if (q < N) t = tail_products<T, D>(oa, half, mse, [&](int, int, int d) { return (float)so[(size_t)q * ld + d]; });
    store_block_partial(t, lane, wave, part + ((((size_t)cell * 2 + dir) * gridDim.y + bh) * qt + qtile) * 4);
}

// pair_finish_kernel over n items (pairs or cells) of nblk partials per direction
int launch_finish(const float* part, int n, int nblk, int mse, double count, float* out, int32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(pair_finish_kernel<false>, dim3((n + 63) / 64), dim3(64), 0, s, part, (const int32_t*)nullptr,
                       (const int32_t*)nullptr, (const int32_t*)nullptr, n, nblk, mse, count, out, status);
    DSIM_HIP_CHECK(hipGetLastError());
    return DSIM_OK;
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
        return launch_finish((const float*)a.scratch, a.n_pairs, qt * a.B * a.H, a.similarity, (double)a.B * a.H * a.N * Dc, out, status, s);
    });
}

// workspace of the tiled score matrix: [self A | self B | partials], each 256-byte aligned
size_t mat_self_bytes(int n, int B, int H, int N, int D, int es) { return up256((size_t)n * B * N * H * D * es); }
size_t mat_part_bytes(long n_cells, int B, int H, int N) { return up256((size_t)n_cells * 2 * B * H * ((N + 127) / 128) * 4 * sizeof(float)); }

template <typename T>
int launch_matrix_t(const void* qa, const void* ka, const void* va, int n_a, const void* qb, const void* kb, const void* vb, int n_b, int B,
                    int H, int N, int D, int mse, float* out, int32_t* status, void* scratch, hipStream_t s) {
    MatArgs m;
    m.q[0] = qa; m.k[0] = ka; m.v[0] = va; m.q[1] = qb; m.k[1] = kb; m.v[1] = vb;
    m.self[0] = scratch;
    m.self[1] = (char*)scratch + mat_self_bytes(n_a, B, H, N, D, sizeof(T));
    m.n_a = n_a; m.n_b = n_b; m.B = B; m.H = H; m.N = N;
    float* part = (float*)((char*)m.self[1] + mat_self_bytes(n_b, B, H, N, D, sizeof(T)));
    return with_head_dim(D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        const int qt = (N + 127) / 128, nc = n_a * n_b;
        int st = launch_lds<matrix_tail_kernel<T, Dc>>(dim3(qt, B * H, n_a + n_b), dim3(256), LDS, s, m, scale_log2_of(Dc), mse, 1, part);
        if (st != DSIM_OK) return st;
        st = launch_lds<matrix_tail_kernel<T, Dc>>(dim3(qt * nc * 2, B * H), dim3(256), LDS, s, m, scale_log2_of(Dc), mse, 0, part);
        if (st != DSIM_OK) return st;
        return launch_finish(part, nc, qt * B * H, mse, (double)B * H * N * Dc, out, status, s);
    });
}

// ---- similarity maps: the score tail kept per token ------------------------------------------------------------------------------
// The score of direction a->b splits over query tokens: cos(O_ab, O_aa) = sum_i dot_i / (|O_ab| |O_aa|) and
// mse = sum_i sqd_i / (B H N D), where dot_i / sqd_i sum over the CFG batch, the heads and d at token i.
// pair_map_kernel is pair_tail_body with the per-token epilogue: pair_tail_kernel's grid, attentions, rounding and products, so that
// a pair's map contributions sum to its score.
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void pair_map_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                        const T* __restrict__ vg, const int32_t* __restrict__ idx_a,
                                                        const int32_t* __restrict__ idx_b, int B, int H, int N,
                                                        float scale_log2, int mse, float* __restrict__ part) {
    pair_tail_body<T, D, true, RowsInOrder>(qg, kg, vg, nullptr, nullptr, idx_a, idx_b, B, H, N, scale_log2, mse, part);
}

// one workgroup per pair, both directions: per token, a fixed-order f64 fold of the B*H partials; over tokens, per-thread strided
// sums and a fixed-order tree.  local: the token's own cosine (|.| of the token's vectors) or mean squared difference; contrib: its
// share of the direction's score, so that 0.5 (sum contrib[0] + sum contrib[1]) is the pair's score (tail_core.h's finish
// arithmetic, as pair_finish_kernel)
constexpr int MAP_FINISH_THREADS = 256;
__global__ __launch_bounds__(MAP_FINISH_THREADS) void pair_map_finish_kernel(const float* __restrict__ part, int BH, int N, int D, int mse,
                                                                             float* __restrict__ score, float* __restrict__ local,
                                                                             float* __restrict__ contrib, int32_t* __restrict__ status) {
    constexpr int NT = MAP_FINISH_THREADS;
    __shared__ double red[3][NT];
    const int p = blockIdx.x, t = threadIdx.x;
    const size_t plane = (size_t)BH * N;
    double res = 0.0;
    for (int dir = 0; dir < 2; ++dir) {
        const float* pd = part + ((size_t)p * 2 + dir) * 3 * plane;
        float* lo = local ? local + ((size_t)p * 2 + dir) * N : nullptr;
        float* co = contrib ? contrib + ((size_t)p * 2 + dir) * N : nullptr;
        auto fold = [&](int comp, int i) {
            double a = 0.0;
            for (int j = 0; j < BH; ++j) a += pd[comp * plane + (size_t)j * N + i];
            return a;
        };
        // pass 1: local, and the direction's squared norms (cosine)
        double x2t = 0.0, y2t = 0.0;
        for (int i = t; i < N; i += NT) {
            const double a = fold(0, i);
            if (mse) {                   // (mse folds no norms)
                if (lo) lo[i] = (float)direction_value(a, 0.0, 0.0, mse, (double)BH * D);
            } else {
                const double x2 = fold(1, i), y2 = fold(2, i);
                x2t += x2; y2t += y2;
                if (lo) lo[i] = (float)direction_value(a, x2, y2, mse, (double)BH * D);
            }
        }
        red[1][t] = x2t; red[2][t] = y2t;
        __syncthreads();
        for (int s = NT / 2; s > 0; s >>= 1) {
            if (t < s) { red[1][t] += red[1][t + s]; red[2][t] += red[2][t + s]; }
            __syncthreads();
        }
        const double den = direction_denominator(red[1][0], red[2][0], mse, (double)BH * N * D);
        // pass 2: contrib (the same fold again: the per-token sums are not kept), and the direction's total
        double ct = 0.0;
        for (int i = t; i < N; i += NT) {
            const double c = fold(0, i) / den;
            ct += c;
            if (co) co[i] = (float)c;
        }
        __syncthreads();                 // (every thread has read red[1..2][0])
        red[0][t] = ct;
        __syncthreads();
        for (int s = NT / 2; s > 0; s >>= 1) {
            if (t < s) red[0][t] += red[0][t + s];
            __syncthreads();
        }
        res += red[0][0];
        __syncthreads();
    }
    if (t == 0) store_score(res, score + p, status ? status + p : nullptr);
}

template <typename T>
int launch_maps_t(const PairArgs& a, float* score, float* local, float* contrib, int32_t* status, hipStream_t s) {
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        const int st = launch_lds<pair_map_kernel<T, Dc>>(dim3((a.N + 127) / 128, a.B * a.H, a.n_pairs * 2), dim3(256), LDS, s,
                                                          (const T*)a.q, (const T*)a.k, (const T*)a.v, a.idx_a, a.idx_b, a.B, a.H, a.N,
                                                          scale_log2_of(Dc), a.similarity, (float*)a.scratch);
        if (st != DSIM_OK) return st;
        hipLaunchKernelGGL(pair_map_finish_kernel, dim3(a.n_pairs), dim3(MAP_FINISH_THREADS), 0, s, (const float*)a.scratch, a.B * a.H,
                           a.N, Dc, a.similarity, score, local, contrib, status);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
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

size_t score_matrix_scratch_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    if (n_a < 1 || n_b < 1 || B < 1 || H < 1 || N < 1 || D < 1) return 0;
    if ((dtype == DSIM_BF16 || dtype == DSIM_F16) && pair_score160_applies(N, D, DSIM_H16))
        return score_matrix160_scratch_bytes(n_a, n_b, B, H);           // (the fp16 persistent kernel has the bf16 one's layout)
    const int es = dtype == DSIM_F32 ? 4 : 2;
    return mat_self_bytes(n_a, B, H, N, D, es) + mat_self_bytes(n_b, B, H, N, D, es) + mat_part_bytes((long)n_a * n_b, B, H, N);
}

int launch_score_matrix(const void* qa, const void* ka, const void* va, int n_a, const void* qb, const void* kb, const void* vb, int n_b,
                        int B, int H, int N, int D, int dtype, int similarity, float* out, int32_t* status, void* scratch,
                        size_t scratch_bytes, hipStream_t s) {
    if (n_a < 1 || n_b < 1 || B < 1 || H < 1 || N < 1 || D % 8 || (similarity != 0 && similarity != 1)) return DSIM_ERR_INVALID;
    if (dtype != DSIM_F32 && dtype != DSIM_BF16 && dtype != DSIM_F16) return DSIM_ERR_INVALID;
    // 32-bit grid extents and cell indices
    const long units = (long)n_a * n_b * 2 * ((N + 127) / 128);
    if (units >= (1l << 31) || (long)n_a * n_b * B * H * 16 >= (1l << 31) || n_a + n_b > 65535) return DSIM_ERR_INVALID;
    if (scratch_bytes < score_matrix_scratch_bytes(n_a, n_b, B, H, N, D, dtype)) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype,
        [&](auto e) {
            typedef typename decltype(e)::type T;
            if constexpr (sizeof(T) == 2)
                if (pair_score160_applies(N, D, DSIM_H16))
                    return launch_score_matrix160(qa, ka, va, n_a, qb, kb, vb, n_b, B, H, similarity, out, status, scratch, scratch_bytes, s);
            return launch_matrix_t<T>(qa, ka, va, n_a, qb, kb, vb, n_b, B, H, N, D, similarity, out, status, scratch, s);
        },
        [&] {
            return DSIM_F16_TWIN(launch_score_matrix(qa, ka, va, n_a, qb, kb, vb, n_b, B, H, N, D, dtype, similarity, out, status, scratch,
                                                     scratch_bytes, s));
        });
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
