// The feature-cosine metrics: the cosine of the tapped self-attention's own output -- the reference's `diffeats`
// (metrics/diffeats.py:136-205: F = to_out.0(attn1's SDPA) + bias over both CFG halves, min-max normalised per image) and
// `dinofeats` (metrics/dino.py:163-183: F = the context layer of Dinov2SelfAttention, class token included, as it is).
//  * feat_attend_kernel:  one self attention per (image, b, h, 128 queries) on the tiled core (attn_core.h's attend, tail_core.h's
//                         settle and fold_rounded: the pair tail's arithmetic and rounding), O as [n][B][N][C] rows in the compute dtype.
//  * nt_gemm_kernel:      C = X Y^T for two row-major operands with K contiguous, one 32 x 128 tile per workgroup (a 32 x 32 MFMA tile
//                         per wave), both operands staged through a double-buffered LDS image 128 bytes of K at a time.  Two uses:
//                         the projection P = O W^T + b (all of K in one workgroup, rounded once to the compute dtype) and the Gram
//                         product of a score matrix (K split over workgroups in GRAM_KCHUNK elements, f32 partials to the workspace).
//                         An output element's K order is fixed by the tile shape alone; rows past an operand's end are zeros.
//  * feat_stats_kernel / feat_normalise_kernel / feat_fold_kernel: per image, min, max and sum of squares of the rounded values
//                         (f32 per workgroup in a fixed order, f64 across workgroups), and (x - mn) / (mx - mn) in f32, rounded.
//  * feat_pair_dot_kernel / feat_pair_finish_kernel: a pair's dot product, f32 per workgroup, f64 across, tail_core.h's cosine finish.
//  * gram_finish_kernel:  a cell's split-K partials folded in f64 in ascending K order, the same cosine finish.
//                         (dsim_feature_matrix_chunked: the same two kernels with the caller's chunk in place of GRAM_KCHUNK.)
// No atomics; an image's features and stats, a pair's score and a cell's value do not depend on what else the call carries.
// Compiled once per 16-bit type; the C entry points live in the bf16 object.
#include "tail_core.h"

namespace dsim {

struct FeatArgs {
    const void* q = nullptr; const void* k = nullptr; const void* v = nullptr;      // [n][B][N][H*D]
    int n = 0, B = 0, H = 0, N = 0, D = 0, L = 0;                                   // L = B N H D: an image's elements
    const void* w_out = nullptr;                                                     // [C][C] compute dtype, or null: no projection
    const float* bias = nullptr;                                                     // [C] f32 (with w_out)
    int minmax = 0;
    void* feats = nullptr;                                                           // [n][B][N][C] compute dtype
    float* stats = nullptr;                                                          // [n][4] f32: sum of squares, min, max, 0
    void* scratch = nullptr; size_t scratch_bytes = 0;                               // 256-byte aligned
};

// this source's own host entry points, per 16-bit type as h16_api.h's (declared here: no other source calls them)
#define DSIM_FEATS_API                                                                                                                  \
    size_t attn_features_scratch_bytes(int n, int B, int H, int N, int D, int L, int dtype, int proj);      /* 0: call not served */   \
    int launch_attn_features(const FeatArgs& a, int dtype, hipStream_t s);                                                              \
    int launch_feature_pair_score(const void* feats, const float* stats, const int32_t* idx_a, const int32_t* idx_b, int n_pairs,      \
                                  int L, int dtype, float* out, int32_t* status, void* scratch, hipStream_t s);                         \
    int launch_feature_matrix(const void* fa, const float* stats_a, int n_a, const void* fb, const float* stats_b, int n_b, int L,      \
                              int dtype, float* out, int32_t* status, void* scratch, hipStream_t s, int kchunk);
inline namespace DSIM_H16_NS {
DSIM_FEATS_API
}
#if !defined(DSIM_H16_IS_F16) && !defined(DSIM_DEVTOOLS)
namespace f16 {
DSIM_FEATS_API
}
#endif

namespace {

constexpr int FCH = 16384;            // elements of an image per workgroup of the streaming kernels (stats, normalise, pair dot)
constexpr int GM = 32, GN = 128;      // nt_gemm_kernel's tile: rows of X, rows of Y
constexpr int G_ROWB = 128;           // bytes of K per row and stage
constexpr int G_RS = G_ROWB + 16;     // LDS row stride: an odd number of 16-byte slots (ds_read_b128)
constexpr int G_STAGE = (GM + GN) * G_RS;
constexpr int GRAM_KCHUNK = 16384;    // elements of K per workgroup of the Gram product (a multiple of a stage's K in every dtype)

// grid (ceil(N/128), B*H, n)
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void feat_attend_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                          const T* __restrict__ vg, int B, int H, int N, float scale_log2,
                                                          T* __restrict__ og) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
    const int ld = H * D;
    const size_t base = (size_t)blockIdx.z * B * N * ld + (size_t)b * N * ld + h * D;
    const int t = blockIdx.x * 128 + wave * 32 + l31;          // query position
    const int q = t < N ? t : N - 1;                           // its row (a position past the end: the last one's)
    QFrags<T, D> qf;
    load_q<T, D>(qf, qg + base + (size_t)q * ld, half, scale_log2);
    OAcc<T, D> oa;
    attend<T, D, false>(qf, kg + base, vg + base, ld, N, smem, oa);
    settle<T, D>(oa);
    T* so = og + base;
    if (t < N) fold_rounded<T, D>(oa, half, 0, [&](int, int, int, int d, T y) { so[(size_t)t * ld + d] = y; return 0; });      // (no state)
}

// C[m][n] = sum_k X[m][k] Y[n][k], X [M][K] and Y [Nn][K] row-major.  GRAM false: kchunk = K, out[m][n] = (T)(C + bias[n]), ld Nn.
// GRAM true: workgroup z sums k in [z kchunk, (z + 1) kchunk) into part[z][m][n] (f32 [splits][M][Nn]).  K % (16 / sizeof(T)) == 0.
// grid (ceil(M/32), ceil(Nn/128), splits)
template <typename T, bool GRAM>
__global__ __launch_bounds__(256) void nt_gemm_kernel(const T* __restrict__ X, int M, const T* __restrict__ Y, int Nn, int K, int kchunk,
                                                      const float* __restrict__ bias, T* __restrict__ out, float* __restrict__ part) {
    constexpr int ES = sizeof(T), VEC = 16 / ES, BK = G_ROWB / ES, NSLOT = 1 + GN / 32;
    typedef typename FragOf<T>::type Frag;
    __shared__ __attribute__((aligned(16))) char lds[2 * G_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int m0 = blockIdx.x * GM, n0 = blockIdx.y * GN;
    const int kb = blockIdx.z * kchunk, ke = (K - kb < kchunk) ? K : kb + kchunk;
    const int nkt = (ke - kb + BK - 1) / BK;
    // staging: 8 chunks of 16 bytes per row and stage; slot 0 is X's tile (row tid / 8), slots 1 .. 4 are Y's (32 rows each)
    const int c = tid & 7, r8 = tid >> 3;
    const T* src[NSLOT];
    bool ok[NSLOT];
    unsigned loff[NSLOT];
    src[0] = X + (size_t)(m0 + r8) * K + c * VEC;
    ok[0] = m0 + r8 < M;
    loff[0] = (unsigned)(r8 * G_RS + c * 16);
#pragma unroll
    for (int i = 1; i < NSLOT; ++i) {
        const int row = (i - 1) * 32 + r8;
        src[i] = Y + (size_t)(n0 + row) * K + c * VEC;
        ok[i] = n0 + row < Nn;
        loff[i] = (unsigned)((GM + row) * G_RS + c * 16);
    }
    u32x4 st[NSLOT];
    auto load = [&](int kt) {
        const int k = kb + kt * BK;
        const bool in = k + c * VEC < ke;          // (ke and the chunk start are multiples of VEC: a chunk is inside or outside as a whole)
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) {
            const u32x4 z = {0u, 0u, 0u, 0u};
            st[i] = (ok[i] && in) ? *reinterpret_cast<const u32x4*>(src[i] + k) : z;
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    load(0);
    for (int kt = 0; kt < nkt; ++kt) {
        // buffer (kt & 1) was last read in iteration kt - 2; every wave has passed barrier kt - 1 since
        char* buf = lds + (kt & 1) * G_STAGE;
#pragma unroll
        for (int i = 0; i < NSLOT; ++i) *reinterpret_cast<u32x4*>(buf + loff[i]) = st[i];
        __syncthreads();
        if (kt + 1 < nkt) load(kt + 1);
        const char* xr = buf + l31 * G_RS + half * 8 * ES;
        const char* yr = buf + (GM + wave * 32 + l31) * G_RS + half * 8 * ES;
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            Frag xf, yf;
            lload_frag(xf, xr + ks * 16 * ES);
            lload_frag(yf, yr + ks * 16 * ES);
            mma(xf, yf, acc);          // acc[r] = C[m0 + (r & 3) + 8 (r >> 2) + 4 half][n0 + 32 wave + l31]
        }
    }
    const int n = n0 + wave * 32 + l31;
    if (n >= Nn) return;
    float bv = 0.f;
    if constexpr (!GRAM) bv = bias[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m >= M) continue;
        if constexpr (GRAM) part[((size_t)blockIdx.z * M + m) * Nn + n] = acc[r];
        else out[(size_t)m * Nn + n] = (T)(acc[r] + bv);
    }
}

// a workgroup's (sum, min, max) folded over its 4 waves (shuffles, then the waves in a fixed order) into o[0..3] = (ss, mn, mx, 0)
__device__ __forceinline__ void store_block_stats(float ss, float mn, float mx, int lane, int wave, float* __restrict__ o) {
    __shared__ float red[4][3];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ss += __shfl_xor(ss, off);
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    if (lane == 0) { red[wave][0] = ss; red[wave][1] = mn; red[wave][2] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        o[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
        o[1] = fminf(fminf(red[0][1], red[1][1]), fminf(red[2][1], red[3][1]));
        o[2] = fmaxf(fmaxf(red[0][2], red[1][2]), fmaxf(red[2][2], red[3][2]));
        o[3] = 0.f;
    }
}

// FCH elements of image blockIdx.y: f(vector of 16 bytes at element e) for this thread's vectors in ascending order
template <typename T, typename F>
__device__ __forceinline__ void for_each_vec(int L, F&& f) {
    constexpr int VEC = 16 / sizeof(T);
    const int e0 = blockIdx.x * FCH + threadIdx.x * VEC;
#pragma unroll 4
    for (int it = 0; it < FCH / (256 * VEC); ++it) {
        const int e = e0 + it * 256 * VEC;
        if (e < L) f(e);          // (L % VEC == 0)
    }
}

// part[image][block] = (sum of squares, min, max, 0) of the block's values.  grid (ceil(L / FCH), n)
template <typename T>
__global__ __launch_bounds__(256) void feat_stats_kernel(const T* __restrict__ x, int L, float* __restrict__ part) {
    constexpr int VEC = 16 / sizeof(T);
    typedef T VecT __attribute__((ext_vector_type(VEC)));
    const T* xi = x + (size_t)blockIdx.y * L;
    float ss = 0.f, mn = INFINITY, mx = -INFINITY;
    for_each_vec<T>(L, [&](int e) {
        const VecT xv = *(const VecT*)(xi + e);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float f = (float)xv[j];
            ss = fmaf(f, f, ss);
            mn = fminf(mn, f);
            mx = fmaxf(mx, f);
        }
    });
    store_block_stats(ss, mn, mx, threadIdx.x & 63, threadIdx.x >> 6, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4);
}

// x <- (T)((x - mn) / (mx - mn)) in place with the image's (mn, mx) of stats; part[image][block][0] = the new values' sum of squares.
// mx == mn: 0 / 0, every value NaN, as the reference's division gives.  grid (ceil(L / FCH), n)
template <typename T>
__global__ __launch_bounds__(256) void feat_normalise_kernel(T* __restrict__ x, int L, const float* __restrict__ stats,
                                                             float* __restrict__ part) {
    constexpr int VEC = 16 / sizeof(T);
    typedef T VecT __attribute__((ext_vector_type(VEC)));
    T* xi = x + (size_t)blockIdx.y * L;
    const float mn = stats[blockIdx.y * 4 + 1], den = stats[blockIdx.y * 4 + 2] - mn;
    float ss = 0.f;
    for_each_vec<T>(L, [&](int e) {
        VecT xv = *(const VecT*)(xi + e);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const T g = (T)(((float)xv[j] - mn) / den);
            xv[j] = g;
            ss = fmaf((float)g, (float)g, ss);
        }
        *(VecT*)(xi + e) = xv;
    });
    store_block_stats(ss, 0.f, 0.f, threadIdx.x & 63, threadIdx.x >> 6, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4);
}

// one thread per image: the f64 fold of its nblk partials in a fixed order into stats[i] = (ss, mn, mx, 0); ss_only keeps mn and mx
__global__ void feat_fold_kernel(const float* __restrict__ part, int n, int nblk, int ss_only, float* __restrict__ stats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* o = part + (size_t)i * nblk * 4;
    double ss = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int j = 0; j < nblk; ++j) { ss += o[4 * j]; mn = fminf(mn, o[4 * j + 1]); mx = fmaxf(mx, o[4 * j + 2]); }
    stats[4 * i] = (float)ss;
    if (!ss_only) { stats[4 * i + 1] = mn; stats[4 * i + 2] = mx; stats[4 * i + 3] = 0.f; }
}

// part[pair][block][0] = the block's share of the dot product of the pair's two images.  grid (ceil(L / FCH), n_pairs)
template <typename T>
__global__ __launch_bounds__(256) void feat_pair_dot_kernel(const T* __restrict__ x, const int32_t* __restrict__ idx_a,
                                                            const int32_t* __restrict__ idx_b, int L, float* __restrict__ part) {
    constexpr int VEC = 16 / sizeof(T);
    typedef T VecT __attribute__((ext_vector_type(VEC)));
    const T* xa = x + (size_t)idx_a[blockIdx.y] * L;
    const T* xb = x + (size_t)idx_b[blockIdx.y] * L;
    TailSums s;
    for_each_vec<T>(L, [&](int e) {
        const VecT av = *(const VecT*)(xa + e), bv = *(const VecT*)(xb + e);
#pragma unroll
        for (int j = 0; j < VEC; ++j) s.s0 = fmaf((float)av[j], (float)bv[j], s.s0);
    });
    store_block_partial(s, threadIdx.x & 63, threadIdx.x >> 6, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4);
}

// the cosine of a dot product and two squared norms with tail_core.h's eps arithmetic (store_score halves: a pair tail's score is
// the mean of two directions)
__device__ __forceinline__ void store_cosine(double dot, double x2, double y2, float* __restrict__ out, int32_t* __restrict__ status) {
    store_score(2.0 * direction_value(dot, x2, y2, 0, 0.0), out, status);
}

// one thread per pair: the f64 fold of its nblk partials in a fixed order, then the cosine against the images' squared norms
__global__ void feat_pair_finish_kernel(const float* __restrict__ part, const float* __restrict__ stats, const int32_t* __restrict__ idx_a,
                                        const int32_t* __restrict__ idx_b, int n_pairs, int nblk, float* __restrict__ out,
                                        int32_t* __restrict__ status) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const float* o = part + (size_t)p * nblk * 4;
    double dot = 0.0;
    for (int j = 0; j < nblk; ++j) dot += o[4 * j];
    store_cosine(dot, stats[4 * idx_a[p]], stats[4 * idx_b[p]], out + p, status ? status + p : nullptr);
}

// one thread per cell: the f64 fold of its split-K partials in ascending K order, then the cosine
__global__ void gram_finish_kernel(const float* __restrict__ part, const float* __restrict__ stats_a, const float* __restrict__ stats_b,
                                   int n_a, int n_b, int splits, float* __restrict__ out, int32_t* __restrict__ status) {
    const size_t cells = (size_t)n_a * n_b, cell = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= cells) return;
    double dot = 0.0;
    for (int z = 0; z < splits; ++z) dot += part[z * cells + cell];
    const int ia = (int)(cell / n_b), ib = (int)(cell - (size_t)ia * n_b);
    store_cosine(dot, stats_a[4 * ia], stats_b[4 * ib], out + cell, status ? status + cell : nullptr);
}

inline int blocks_of(int L) { return (L + FCH - 1) / FCH; }
inline int splits_of(int L, int kchunk = GRAM_KCHUNK) { return (L + kchunk - 1) / kchunk; }
// a caller's K chunk (dsim_feature_matrix_chunked): whole stages of every dtype, no longer than the default
inline bool kchunk_ok(int kchunk) { return kchunk >= 64 && kchunk <= GRAM_KCHUNK && kchunk % 64 == 0; }
inline bool dtype_ok(int dtype) { return dtype == DSIM_F32 || dtype == DSIM_BF16 || dtype == DSIM_F16; }

// an image's length: 16-byte vectors in every dtype, 32-bit element offsets inside an image (a last block's end included)
inline bool length_ok(long L) { return L >= 8 && L % 8 == 0 && L <= (1l << 30); }

// workspace of dsim_attn_features: [the O slab [n][L] (projection only) |] partials f32 [n][blocks][4], each 256-byte aligned
struct FeatLayout {
    size_t slab, parts;
    FeatLayout(int n, int L, size_t es, bool proj) : slab(proj ? up256((size_t)n * L * es) : 0), parts(up256((size_t)n * blocks_of(L) * 16)) {}
    size_t total() const { return slab + parts; }
};

bool features_served(int n, int B, int H, int N, int D, int L, int dtype) {
    if (!dtype_ok(dtype) || n < 1 || n > 65535 || B < 1 || H < 1 || N < 1) return false;
    if (with_head_dim(D, [](auto) { return DSIM_OK; }) != DSIM_OK) return false;
    if ((long)B * H > 65535 || (long)B * N * H * D != (long)L || !length_ok(L)) return false;
    return (long)n * B * N < (1l << 31);          // the projection's rows
}

template <typename T>
int launch_features_t(const FeatArgs& a, hipStream_t s) {
    const bool proj = a.w_out != nullptr;
    const FeatLayout lay(a.n, a.L, sizeof(T), proj);
    T* feats = (T*)a.feats;
    T* o = proj ? (T*)a.scratch : feats;
    float* part = (float*)((char*)a.scratch + lay.slab);
    const int C = a.H * a.D, nblk = blocks_of(a.L);
    int st = with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        return launch_lds<feat_attend_kernel<T, Dc>>(dim3((a.N + 127) / 128, a.B * a.H, a.n), dim3(256), LDS, s, (const T*)a.q, (const T*)a.k,
                                                     (const T*)a.v, a.B, a.H, a.N, scale_log2_of(Dc), o);
    });
    if (st != DSIM_OK) return st;
    if (proj) {
        const int M = a.n * a.B * a.N;
        hipLaunchKernelGGL((nt_gemm_kernel<T, false>), dim3((M + GM - 1) / GM, (C + GN - 1) / GN, 1), dim3(256), 0, s, (const T*)o, M,
                           (const T*)a.w_out, C, C, C, a.bias, feats, (float*)nullptr);
        DSIM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(feat_stats_kernel<T>, dim3(nblk, a.n), dim3(256), 0, s, (const T*)feats, a.L, part);
    hipLaunchKernelGGL(feat_fold_kernel, dim3((a.n + 63) / 64), dim3(64), 0, s, (const float*)part, a.n, nblk, 0, a.stats);
    if (a.minmax) {
        hipLaunchKernelGGL(feat_normalise_kernel<T>, dim3(nblk, a.n), dim3(256), 0, s, feats, a.L, (const float*)a.stats, part);
        hipLaunchKernelGGL(feat_fold_kernel, dim3((a.n + 63) / 64), dim3(64), 0, s, (const float*)part, a.n, nblk, 1, a.stats);
    }
    DSIM_HIP_CHECK(hipGetLastError());
    return DSIM_OK;
}

template <typename T>
int launch_pair_t(const void* feats, const float* stats, const int32_t* idx_a, const int32_t* idx_b, int n_pairs, int L, float* out,
                  int32_t* status, void* scratch, hipStream_t s) {
    const int nblk = blocks_of(L);
    hipLaunchKernelGGL(feat_pair_dot_kernel<T>, dim3(nblk, n_pairs), dim3(256), 0, s, (const T*)feats, idx_a, idx_b, L, (float*)scratch);
    hipLaunchKernelGGL(feat_pair_finish_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, s, (const float*)scratch, stats, idx_a, idx_b,
                       n_pairs, nblk, out, status);
    DSIM_HIP_CHECK(hipGetLastError());
    return DSIM_OK;
}

template <typename T>
int launch_gram_t(const void* fa, const float* stats_a, int n_a, const void* fb, const float* stats_b, int n_b, int L, float* out,
                  int32_t* status, void* scratch, hipStream_t s, int kchunk) {
    const int splits = splits_of(L, kchunk);
    hipLaunchKernelGGL((nt_gemm_kernel<T, true>), dim3((n_a + GM - 1) / GM, (n_b + GN - 1) / GN, splits), dim3(256), 0, s, (const T*)fa, n_a,
                       (const T*)fb, n_b, L, kchunk, (const float*)nullptr, (T*)nullptr, (float*)scratch);
    const size_t cells = (size_t)n_a * n_b;
    hipLaunchKernelGGL(gram_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, (const float*)scratch, stats_a, stats_b,
                       n_a, n_b, splits, out, status);
    DSIM_HIP_CHECK(hipGetLastError());
    return DSIM_OK;
}

}  // namespace

inline namespace DSIM_H16_NS {
size_t attn_features_scratch_bytes(int n, int B, int H, int N, int D, int L, int dtype, int proj) {
    if (!features_served(n, B, H, N, D, L, dtype)) return 0;
    return FeatLayout(n, L, dtype_size(dtype), proj != 0).total();
}

int launch_attn_features(const FeatArgs& a, int dtype, hipStream_t s) {
    return by_h16_dtype(
        dtype, [&](auto e) { return launch_features_t<typename decltype(e)::type>(a, s); },
        [&] { return DSIM_F16_TWIN(launch_attn_features(a, dtype, s)); });
}

int launch_feature_pair_score(const void* feats, const float* stats, const int32_t* idx_a, const int32_t* idx_b, int n_pairs, int L,
                              int dtype, float* out, int32_t* status, void* scratch, hipStream_t s) {
    return by_h16_dtype(
        dtype,
        [&](auto e) { return launch_pair_t<typename decltype(e)::type>(feats, stats, idx_a, idx_b, n_pairs, L, out, status, scratch, s); },
        [&] { return DSIM_F16_TWIN(launch_feature_pair_score(feats, stats, idx_a, idx_b, n_pairs, L, dtype, out, status, scratch, s)); });
}

int launch_feature_matrix(const void* fa, const float* stats_a, int n_a, const void* fb, const float* stats_b, int n_b, int L, int dtype,
                          float* out, int32_t* status, void* scratch, hipStream_t s, int kchunk) {
    return by_h16_dtype(
        dtype,
        [&](auto e) { return launch_gram_t<typename decltype(e)::type>(fa, stats_a, n_a, fb, stats_b, n_b, L, out, status, scratch, s, kchunk); },
        [&] { return DSIM_F16_TWIN(launch_feature_matrix(fa, stats_a, n_a, fb, stats_b, n_b, L, dtype, out, status, scratch, s, kchunk)); });
}
}  // namespace DSIM_H16_NS

}  // namespace dsim

#ifndef DSIM_H16_IS_F16
using namespace dsim;

namespace {
// the workspace from its first 256-byte boundary: false when `need` bytes do not fit behind it
bool aligned_workspace(void* workspace, size_t bytes, size_t need, void** at) {
    const size_t lost = (size_t)(-(uintptr_t)workspace & 255);
    if (bytes < lost || bytes - lost < need) return false;
    *at = (char*)workspace + lost;
    return true;
}
size_t pair_scratch(int n_pairs, int L, int dtype) {
    if (!dtype_ok(dtype) || n_pairs < 1 || n_pairs > 65535 || !length_ok(L)) return 0;
    return up256((size_t)n_pairs * blocks_of(L) * 16);
}
size_t matrix_scratch(int n_a, int n_b, int L, int dtype, int kchunk = GRAM_KCHUNK) {
    if (!dtype_ok(dtype) || n_a < 1 || n_b < 1 || !length_ok(L) || !kchunk_ok(kchunk)) return 0;
    if ((long)n_a * n_b >= (1l << 31) || (n_b + GN - 1) / GN > 65535) return 0;      // the cells; the column tiles' grid axis
    if (splits_of(L, kchunk) > 65535) return 0;                                       // the splits' grid axis
    return up256((size_t)splits_of(L, kchunk) * n_a * n_b * sizeof(float));
}
}  // namespace

extern "C" {

size_t dsim_attn_features_workspace_bytes(int n, int B, int H, int N, int D, int L, int dtype, int proj) {
    const size_t b = attn_features_scratch_bytes(n, B, H, N, D, L, dtype, proj);
    return b ? b + 256 : 0;
}

int dsim_attn_features(const void* q, const void* k, const void* v, int n, int B, int H, int N, int D, int L, int dtype, const void* w_out,
                       const float* bias, int minmax, void* feats, float* stats, void* workspace, size_t workspace_bytes, void* stream) {
    if (!q || !k || !v || !feats || !stats || !workspace || (w_out != nullptr) != (bias != nullptr)) return DSIM_ERR_INVALID;
    const size_t need = attn_features_scratch_bytes(n, B, H, N, D, L, dtype, w_out != nullptr);
    if (need == 0) return DSIM_ERR_INVALID;
    FeatArgs a;
    a.q = q; a.k = k; a.v = v; a.n = n; a.B = B; a.H = H; a.N = N; a.D = D; a.L = L;
    a.w_out = w_out; a.bias = bias; a.minmax = minmax != 0; a.feats = feats; a.stats = stats;
    if (!aligned_workspace(workspace, workspace_bytes, need, &a.scratch)) return DSIM_ERR_WORKSPACE;
    a.scratch_bytes = need;
    return launch_attn_features(a, dtype, (hipStream_t)stream);
}

size_t dsim_feature_pair_score_workspace_bytes(int n_pairs, int L, int dtype) {
    const size_t b = pair_scratch(n_pairs, L, dtype);
    return b ? b + 256 : 0;
}

int dsim_feature_pair_score(const void* feats, const float* stats, const int32_t* idx_a, const int32_t* idx_b, int n_pairs, int L, int dtype,
                            float* out_scores, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (!feats || !stats || !idx_a || !idx_b || !out_scores || !workspace) return DSIM_ERR_INVALID;
    const size_t need = pair_scratch(n_pairs, L, dtype);
    if (need == 0) return DSIM_ERR_INVALID;
    void* scratch;
    if (!aligned_workspace(workspace, workspace_bytes, need, &scratch)) return DSIM_ERR_WORKSPACE;
    return launch_feature_pair_score(feats, stats, idx_a, idx_b, n_pairs, L, dtype, out_scores, status, scratch, (hipStream_t)stream);
}

size_t dsim_feature_matrix_workspace_bytes(int n_a, int n_b, int L, int dtype) {
    const size_t b = matrix_scratch(n_a, n_b, L, dtype);
    return b ? b + 256 : 0;
}

int dsim_feature_matrix(const void* fa, const float* stats_a, int n_a, const void* fb, const float* stats_b, int n_b, int L, int dtype,
                        float* out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (!fa || !stats_a || !fb || !stats_b || !out || !workspace) return DSIM_ERR_INVALID;
    const size_t need = matrix_scratch(n_a, n_b, L, dtype);
    if (need == 0) return DSIM_ERR_INVALID;
    void* scratch;
    if (!aligned_workspace(workspace, workspace_bytes, need, &scratch)) return DSIM_ERR_WORKSPACE;
    return launch_feature_matrix(fa, stats_a, n_a, fb, stats_b, n_b, L, dtype, out, status, scratch, (hipStream_t)stream, GRAM_KCHUNK);
}

size_t dsim_feature_matrix_chunked_workspace_bytes(int n_a, int n_b, int L, int dtype, int k_chunk) {
    const size_t b = matrix_scratch(n_a, n_b, L, dtype, k_chunk);
    return b ? b + 256 : 0;
}

int dsim_feature_matrix_chunked(const void* fa, const float* stats_a, int n_a, const void* fb, const float* stats_b, int n_b, int L,
                                int dtype, int k_chunk, float* out, int32_t* status, void* workspace, size_t workspace_bytes,
                                void* stream) {
    if (!fa || !stats_a || !fb || !stats_b || !out || !workspace) return DSIM_ERR_INVALID;
    const size_t need = matrix_scratch(n_a, n_b, L, dtype, k_chunk);
    if (need == 0) return DSIM_ERR_INVALID;
    void* scratch;
    if (!aligned_workspace(workspace, workspace_bytes, need, &scratch)) return DSIM_ERR_WORKSPACE;
    return launch_feature_matrix(fa, stats_a, n_a, fb, stats_b, n_b, L, dtype, out, status, scratch, (hipStream_t)stream, k_chunk);
}

}  // extern "C"
#endif
