// The fused DiffSim score tails on the tiled attention core (attn_core.h), for any shape and compute dtype; the default tap's
// persistent kernels are attn160.hip's.
//
//  * pair_tail_kernel: the DiffSim score tail -- /root/reference/diffsim/diffsim.py:177-197:
//                      O_ab = SDPA(Qa,Kb,Vb), O_aa = SDPA(Qa,Ka,Va) (and the b<->a mirror), then
//                      cosine (or mse) over the flattened (B,H,N,D) tensors.  Both attentions of a
//                      direction share Q and run in one workgroup; O never leaves registers, only
//                      three f32 partial sums per workgroup reach HBM and a second fixed-order pass
//                      folds them (no float atomics => bit-reproducible scores).
#include "tail_core.h"

namespace dsim {
namespace {

// One direction of a pair in a 128-query workgroup: the self and the cross attention on the same Q fragments, then their products.
// The epilogue is pair_tail_kernel's (PER_TOKEN false: one partial per workgroup, [pair][dir][bh][qtile][4] f32) or pair_map_kernel's
// (PER_TOKEN true: one per query token, [pair][dir][comp][bh][N] f32, comp: dot | x2 | y2, or sqd | - | -).
// grid (ceil(N/128), B*H, n_pairs*2)
template <typename T, int D, bool PER_TOKEN>
__device__ __forceinline__ void pair_tail_body(const T* __restrict__ qg, const T* __restrict__ kg, const T* __restrict__ vg,
                                               const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_b, int B, int H, int N,
                                               float scale_log2, int mse, float* __restrict__ part) {
    typedef ACfg<T, D> C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
    const int pair = blockIdx.z >> 1, dir = blockIdx.z & 1;
    const int ia = idx_a[pair], ib = idx_b[pair];
    const int iq = dir ? ib : ia;        // query image (also the "self" keys/values)
    const int ix = dir ? ia : ib;        // the other image ("cross" keys/values)
    const int ld = H * D;
    const size_t img = (size_t)B * N * ld;
    const int q = blockIdx.x * 128 + wave * 32 + l31;
    const int qc = q < N ? q : N - 1;
    const size_t boff = (size_t)b * N * ld + h * D;
    QFrags<T, D> qf;
    load_q<T, D>(qf, qg + iq * img + boff + (size_t)qc * ld, half, scale_log2);
    TailSums t;
    if constexpr (sizeof(T) == 2) {
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        h16x2 osp[C::NDB][8];           // the self-attention's output, rounded to the compute dtype, two values per register
        {
            OAcc<T, D> osa;
            attend<T, D>(qf, kg + iq * img + boff, vg + iq * img + boff, ld, N, smem, osa);
            settle<T, D>(osa);
#pragma unroll
            for (int db = 0; db < C::NDB; ++db)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    osp[db][r >> 1] = __builtin_convertvector((f32x2){osa.b[db][r], osa.b[db][r + 1]}, h16x2);
                    asm volatile("" : "+v"(osp[db][r >> 1]));          // (pinned: the f32 accumulators die here, before the second attention)
                }
        }
        OAcc<T, D> oxa;
        attend<T, D>(qf, kg + ix * img + boff, vg + ix * img + boff, ld, N, smem, oxa);
        settle<T, D>(oxa);
        if (q < N) t = tail_products<T, D>(oxa, half, mse, [&](int db, int r, int) { return (float)osp[db][r >> 1][r & 1]; });
    } else {
        OAcc<T, D> osa, oxa;
        attend<T, D>(qf, kg + iq * img + boff, vg + iq * img + boff, ld, N, smem, osa);
        attend<T, D>(qf, kg + ix * img + boff, vg + ix * img + boff, ld, N, smem, oxa);
        settle<T, D>(osa);
        settle<T, D>(oxa);
        if (q < N) t = tail_products<T, D>(oxa, half, mse, [&](int db, int r, int) { return osa.b[db][r]; });
    }
    if constexpr (PER_TOKEN) {
        // a row's d values are split between the two lane halves: fold them, then the first half stores the row (128 B per wave and
        // component, no atomics)
        const float s0 = t.s0 + __shfl_xor(t.s0, 32);
        const float s1 = t.s1 + __shfl_xor(t.s1, 32);
        const float s2 = t.s2 + __shfl_xor(t.s2, 32);
        if (half == 0 && q < N) {
            const size_t plane = (size_t)gridDim.y * N;
            float* o = part + ((size_t)pair * 2 + dir) * 3 * plane + (size_t)bh * N + q;
            o[0] = s0;
            if (!mse) { o[plane] = s1; o[2 * plane] = s2; }
        }
    } else {
        store_block_partial(t, lane, wave, part + ((((size_t)pair * 2 + dir) * gridDim.y + bh) * gridDim.x + blockIdx.x) * 4);
    }
}

template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void pair_tail_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                        const T* __restrict__ vg, const int32_t* __restrict__ idx_a,
                                                        const int32_t* __restrict__ idx_b, int B, int H, int N,
                                                        float scale_log2, int mse, float* __restrict__ part) {
    pair_tail_body<T, D, false>(qg, kg, vg, idx_a, idx_b, B, H, N, scale_log2, mse, part);
}

// one thread per pair: fixed-order f64 fold of the partials, then cosine / mse and the mean of
// the two directions (diffsim.py:187-197; F.cosine_similarity eps = 1e-8)
__global__ void pair_finish_kernel(const float* __restrict__ part, int n_pairs, int nblk, int mse, double count,
                                   float* __restrict__ out, int32_t* __restrict__ status) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    double res = 0.0;
    for (int dir = 0; dir < 2; ++dir) {
        double a = 0.0, x2 = 0.0, y2 = 0.0;
        const float* o = part + ((size_t)p * 2 + dir) * nblk * 4;
        for (int i = 0; i < nblk; ++i) { a += o[4 * i]; x2 += o[4 * i + 1]; y2 += o[4 * i + 2]; }
        if (mse) res += a / count;
        else {
            const double nx = sqrt(x2), ny = sqrt(y2);
            res += a / (fmax(nx, 1e-8) * fmax(ny, 1e-8));
        }
    }
    const float sc = (float)(res * 0.5);
    out[p] = sc;
    // NaN guard: non-finite features surface here as a non-finite score; report them per pair
    if (status) status[p] = (sc - sc == 0.0f) ? 0 : 1;
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

template <typename T>
int launch_tail_t(const void* q, const void* k, const void* v, const int32_t* ia, const int32_t* ib, int n_pairs,
                  int B, int H, int N, int D, int mse, float* out, void* scratch, hipStream_t s, int32_t* status) {
    return with_head_dim(D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        const int qt = (N + 127) / 128;
        const int st = launch_lds<pair_tail_kernel<T, Dc>>(dim3(qt, B * H, n_pairs * 2), dim3(256), LDS, s, (const T*)q, (const T*)k,
                                                           (const T*)v, ia, ib, B, H, N, scale_log2_of(Dc), mse, (float*)scratch);
        if (st != DSIM_OK) return st;
        hipLaunchKernelGGL(pair_finish_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, s, (const float*)scratch, n_pairs,
                           qt * B * H, mse, (double)B * H * N * Dc, out, status);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

// workspace of the tiled score matrix: [self A | self B | partials], each 256-byte aligned
size_t mat_self_bytes(int n, int B, int H, int N, int D, int es) { return (((size_t)n * B * N * H * D * es) + 255) & ~(size_t)255; }
size_t mat_part_bytes(long n_cells, int B, int H, int N) { return (((size_t)n_cells * 2 * B * H * ((N + 127) / 128) * 4 * sizeof(float)) + 255) & ~(size_t)255; }

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
        hipLaunchKernelGGL(pair_finish_kernel, dim3((nc + 63) / 64), dim3(64), 0, s, (const float*)part, nc, qt * B * H, mse,
                           (double)B * H * N * Dc, out, status);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
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
    pair_tail_body<T, D, true>(qg, kg, vg, idx_a, idx_b, B, H, N, scale_log2, mse, part);
}

// one workgroup per pair, both directions: per token, a fixed-order f64 fold of the B*H partials; over tokens, per-thread strided
// sums and a fixed-order tree.  local: the token's own cosine (|.| of the token's vectors) or mean squared difference; contrib: its
// share of the direction's score, so that 0.5 (sum contrib[0] + sum contrib[1]) is the pair's score (F.cosine_similarity eps =
// 1e-8, as pair_finish_kernel)
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
            if (mse) {
                if (lo) lo[i] = (float)(a / ((double)BH * D));
            } else {
                const double x2 = fold(1, i), y2 = fold(2, i);
                x2t += x2; y2t += y2;
                if (lo) lo[i] = (float)(a / (fmax(sqrt(x2), 1e-8) * fmax(sqrt(y2), 1e-8)));
            }
        }
        red[1][t] = x2t; red[2][t] = y2t;
        __syncthreads();
        for (int s = NT / 2; s > 0; s >>= 1) {
            if (t < s) { red[1][t] += red[1][t + s]; red[2][t] += red[2][t + s]; }
            __syncthreads();
        }
        const double den = mse ? (double)BH * N * D : fmax(sqrt(red[1][0]), 1e-8) * fmax(sqrt(red[2][0]), 1e-8);
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
    if (t == 0) {
        const float sc = (float)(res * 0.5);
        score[p] = sc;
        if (status) status[p] = (sc - sc == 0.0f) ? 0 : 1;
    }
}

template <typename T>
int launch_maps_t(const void* q, const void* k, const void* v, const int32_t* ia, const int32_t* ib, int n_pairs, int B, int H, int N,
                  int D, int mse, float* score, float* local, float* contrib, int32_t* status, void* scratch, hipStream_t s) {
    return with_head_dim(D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        const int st = launch_lds<pair_map_kernel<T, Dc>>(dim3((N + 127) / 128, B * H, n_pairs * 2), dim3(256), LDS, s, (const T*)q,
                                                          (const T*)k, (const T*)v, ia, ib, B, H, N, scale_log2_of(Dc), mse, (float*)scratch);
        if (st != DSIM_OK) return st;
        hipLaunchKernelGGL(pair_map_finish_kernel, dim3(n_pairs), dim3(MAP_FINISH_THREADS), 0, s, (const float*)scratch, B * H, N, Dc,
                           mse, score, local, contrib, status);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
size_t pair_score_scratch_bytes(int n_pairs, int B, int H, int N, int D) {
    const size_t tiled = (size_t)n_pairs * 2 * B * H * ((N + 127) / 128) * 4 * sizeof(float);
    if (pair_score160_applies(N, D, DSIM_H16)) {          // (dtype-blind: the 16-bit modes' persistent kernel needs the larger workspace)
        const size_t pers = pair_score160_scratch_bytes(n_pairs, B, H);
        return pers > tiled ? pers : tiled;
    }
    return tiled;
}

int launch_pair_score(const void* q, const void* k, const void* v, const int32_t* ia, const int32_t* ib,
                      int n_pairs, int B, int H, int N, int D, int dtype, int similarity, float* out, void* scratch,
                      size_t scratch_bytes, hipStream_t s, int32_t* status) {
    if (n_pairs <= 0 || D % 8 || N < 1) return DSIM_ERR_INVALID;
    if (scratch_bytes < pair_score_scratch_bytes(n_pairs, B, H, N, D)) return DSIM_ERR_WORKSPACE;
    if (n_pairs * 2 > 65535) return DSIM_ERR_INVALID;
    if (dtype == DSIM_H16) {
        if (pair_score160_applies(N, D, DSIM_H16))
            return launch_pair_score160(q, k, v, ia, ib, n_pairs, B, H, similarity, out, scratch, scratch_bytes, s, status);
        return launch_tail_t<h16>(q, k, v, ia, ib, n_pairs, B, H, N, D, similarity, out, scratch, s, status);
    }
#ifndef DSIM_H16_IS_F16
    if (dtype == DSIM_F32) return launch_tail_t<float>(q, k, v, ia, ib, n_pairs, B, H, N, D, similarity, out, scratch, s, status);
    if (dtype == DSIM_F16)
        return DSIM_F16_TWIN(launch_pair_score(q, k, v, ia, ib, n_pairs, B, H, N, D, dtype, similarity, out, scratch, scratch_bytes, s, status));
#endif
    return DSIM_ERR_INVALID;
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
    if (dtype == DSIM_H16) {
        if (pair_score160_applies(N, D, DSIM_H16))
            return launch_score_matrix160(qa, ka, va, n_a, qb, kb, vb, n_b, B, H, similarity, out, status, scratch, scratch_bytes, s);
        return launch_matrix_t<h16>(qa, ka, va, n_a, qb, kb, vb, n_b, B, H, N, D, similarity, out, status, scratch, s);
    }
#ifndef DSIM_H16_IS_F16
    if (dtype == DSIM_F32)
        return launch_matrix_t<float>(qa, ka, va, n_a, qb, kb, vb, n_b, B, H, N, D, similarity, out, status, scratch, s);
    if (dtype == DSIM_F16)
        return DSIM_F16_TWIN(launch_score_matrix(qa, ka, va, n_a, qb, kb, vb, n_b, B, H, N, D, dtype, similarity, out, status, scratch, scratch_bytes, s));
#endif
    return DSIM_ERR_INVALID;
}


size_t pair_score_maps_scratch_bytes(int n_pairs, int B, int H, int N) {
    if (n_pairs < 1 || B < 1 || H < 1 || N < 1) return 0;
    return (size_t)n_pairs * 2 * 3 * B * H * N * sizeof(float);
}

// per-token maps of the score tail: pair_map_kernel at every shape and dtype (the default tap's persistent kernel keeps no
// per-token sums)
int launch_pair_score_maps(const void* q, const void* k, const void* v, const int32_t* ia, const int32_t* ib, int n_pairs, int B, int H,
                           int N, int D, int dtype, int similarity, float* score, float* local, float* contrib, int32_t* status,
                           void* scratch, size_t scratch_bytes, hipStream_t s) {
    if (n_pairs <= 0 || B < 1 || H < 1 || D % 8 || N < 1 || (similarity != 0 && similarity != 1)) return DSIM_ERR_INVALID;
    if (n_pairs * 2 > 65535 || B * H > 65535) return DSIM_ERR_INVALID;
    if (scratch_bytes < pair_score_maps_scratch_bytes(n_pairs, B, H, N)) return DSIM_ERR_WORKSPACE;
    if (dtype == DSIM_H16)
        return launch_maps_t<h16>(q, k, v, ia, ib, n_pairs, B, H, N, D, similarity, score, local, contrib, status, scratch, s);
#ifndef DSIM_H16_IS_F16
    if (dtype == DSIM_F32)
        return launch_maps_t<float>(q, k, v, ia, ib, n_pairs, B, H, N, D, similarity, score, local, contrib, status, scratch, s);
    if (dtype == DSIM_F16)
        return DSIM_F16_TWIN(launch_pair_score_maps(q, k, v, ia, ib, n_pairs, B, H, N, D, dtype, similarity, score, local, contrib, status,
                                                    scratch, scratch_bytes, s));
#endif
    return DSIM_ERR_INVALID;
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
