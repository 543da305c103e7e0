// GroupNorm(+SiLU) and LayerNorm for token-major activations on gfx950 (HBM-bound kernels).
//
// Replaces torch.nn.GroupNorm / F.silu / torch.nn.LayerNorm as used by diffusers'
// ResnetBlock2D, Transformer2DModel and BasicTransformerBlock (SURVEY.md Appendix A items 3-5;
// block control flow: /root/reference/diffsim/hacked_modules.py:39-40, 336-339).
//
// GroupNorm runs as two launches over [B][HW][C] (C = C0+C1: the up-path channel concat
// cat([h, skip]) is read from its two sources and never materialised un-normalised):
//   1. gn_stats : every workgroup streams a slab of rows with 16-byte loads, each thread owning
//                 fixed channel slots; per-channel f32 partials -> fixed-order f64 reduction
//                 per group -> one (sum, sumsq) f64 pair per (batch, slab, group).
//   2. gn_apply : folds the slab partials in fixed order, then y = (x-mean)*rstd*gamma+beta
//                 [*sigmoid] with 16-byte loads and stores.
// launch_groupnorm_stats is the statistics alone: pass 1 (or the one-pass form's own partials and fold where that form serves the
// shape), then gn_coef_kernel writes gn_apply's fold and coefficients once per image for a consumer that normalises the rows it
// holds (rowres.hip, gn_rowlin_kernel).
// No float atomics anywhere: results are bit-reproducible and independent of batch size.
#include <type_traits>

#include "common.h"

namespace dsim {
namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_MAX_SLOTS = 4;     // channel slots (16 B each) a thread may own: C <= 4*256*VEC

// x*sigmoid(x) with the hardware exp2/rcp (1 ulp each): the apply pass is otherwise VALU-bound on libm's expf + divide
__device__ __forceinline__ float silu_fast(float y) {
    return y * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * y));
}

template <typename T> struct Vec16;
template <> struct Vec16<bf16_t> { typedef __attribute__((ext_vector_type(8))) bf16_t type; static constexpr int N = 8; };
template <> struct Vec16<f16_t> { typedef __attribute__((ext_vector_type(8))) f16_t type; static constexpr int N = 8; };
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int N = 4; };

__host__ __device__ inline int gn_chunks(int HW) {
    int c = HW / 64;
    c = c < 1 ? 1 : (c > 32 ? 32 : c);
    if (HW > 16384) c = 64;          // the VAE's 256^2 / 512^2 maps: few images, so more slabs per image
    return c;
}

template <typename T>
__device__ __forceinline__ typename Vec16<T>::type load_slot(const T* x0, int C0, const T* x1, int C1,
                                                             size_t row, int ch) {
    typedef typename Vec16<T>::type V;
    return ch < C0 ? *reinterpret_cast<const V*>(x0 + row * C0 + ch)
                   : *reinterpret_cast<const V*>(x1 + row * C1 + (ch - C0));
}

// full 64-lane xor trees, and the one over the LPR (a power of two <= 64) adjacent lanes that share a row
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float lpr_sum(float v, int LPR) {
    if (LPR > 32) v += __shfl_xor(v, 32);
    if (LPR > 16) v += __shfl_xor(v, 16);
    if (LPR > 8) v += __shfl_xor(v, 8);
    if (LPR > 4) v += __shfl_xor(v, 4);
    if (LPR > 2) v += __shfl_xor(v, 2);
    if (LPR > 1) v += __shfl_xor(v, 1);
    return v;
}

// ---- the f64 (sum, sum of squares) folds.  Their order is what makes a batch of N score bit for bit like N single images: it
// depends on the shape only, and it is written here once.
// xor tree over w (a power of two <= 64) adjacent lanes
__device__ __forceinline__ void gn_pair_tree(double& a, double& q, int w) {
    for (int off = w >> 1; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, 64);
        q += __shfl_xor(q, off, 64);
    }
}
// the per-wave pairs through s_w, then the lead thread of nw consecutive waves sums them in wave order, from wave w0
__device__ __forceinline__ void gn_pair_waves(double (*s_w)[2], int tid, bool lead, int w0, int nw, double& a, double& q) {
    if ((tid & 63) == 0) { s_w[tid >> 6][0] = a; s_w[tid >> 6][1] = q; }
    __syncthreads();
    if (lead) {
        a = 0.0; q = 0.0;
        for (int k = 0; k < nw; ++k) { a += s_w[w0 + k][0]; q += s_w[w0 + k][1]; }
    }
}
// Fold of the R x cpg per-channel f32 partials of each of `ngroups` groups, lds[R][stride][2]: the tg = GN_THREADS / (groups rounded
// up to a power of two) threads of group g take a fixed strided subset each (thread t: partials t, t + tg, ...), then a fixed
// xor-shuffle tree and, where a group is wider than a wave (fewer than 4 groups), a last serial fold of the per-wave sums.  The pair
// of group g is thread t == 0's (a, q).  (One thread per group walking the list serially held the whole workgroup -- and, with every
// workgroup of the launch in the same phase, the chip -- for several microseconds.)  Holds a barrier when tg > 64: uniform calls only.
template <bool RAGGED>      // RAGGED: tg * ngroups may fall short of the workgroup (ngroups no power of two); threads past the last group idle
__device__ __forceinline__ void gn_group_fold(const float* lds, int stride, int R, int cpg, int ngroups, int tg, int tid, int& g,
                                              int& t, double& a, double& q) {
    __shared__ double s_w[GN_THREADS / 64][2];
    g = tid / tg;
    t = tid - g * tg;
    const int cnt = R * cpg;
    a = 0.0; q = 0.0;
    if (!RAGGED || g < ngroups)
        for (int i = t; i < cnt; i += tg) {
            const int rr = i / cpg, c = g * cpg + (i - rr * cpg);
            const float2 pr = *reinterpret_cast<const float2*>(&lds[((size_t)rr * stride + c) * 2]);
            a += (double)pr.x;
            q += (double)pr.y;
        }
    gn_pair_tree(a, q, tg < 64 ? tg : 64);
    if (tg > 64) gn_pair_waves(s_w, tid, t == 0, g * (tg / 64), tg / 64, a, q);
}
__device__ __forceinline__ void gn_mean_rstd(double a, double q, double n, float eps, float* mean, float* rstd) {
    const double m = a / n;
    double var = q / n - m * m;
    if (var < 0.0) var = 0.0;
    *mean = (float)m;
    *rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// The image's chunks x groups partial pairs -> s_mean / s_rstd [groups], the one fold every consumer of gn_stats_kernel's scratch
// shares (gn_apply_kernel, gn_coef_kernel): fetched by the whole workgroup in one round trip (a per-group thread walking them
// serially cost ~32 dependent L2 round trips before the first row was streamed), then 4 threads per group (groups <= 64) take every
// 4th chunk and a two-step xor-shuffle adds them: fixed order per shape.  fold: chunks * groups * 2 doubles of LDS.  Holds barriers.
__device__ __forceinline__ void gn_fold_partials(const double* __restrict__ part, int b, int chunks, int groups, double n, float eps,
                                                 double* fold, float* s_mean, float* s_rstd) {
    const int tid = threadIdx.x;
    {
        const double* src = part + (size_t)b * chunks * groups * 2;
        const int cnt = chunks * groups * 2;
        for (int i = tid; i < cnt; i += GN_THREADS) fold[i] = src[i];
    }
    __syncthreads();
    {
        const int g = tid >> 2, t = tid & 3;
        double a = 0.0, q = 0.0;
        if (g < groups)
            for (int c = t; c < chunks; c += 4) {
                a += fold[(c * groups + g) * 2];
                q += fold[(c * groups + g) * 2 + 1];
            }
        a += __shfl_xor(a, 2, 64); q += __shfl_xor(q, 2, 64);
        a += __shfl_xor(a, 1, 64); q += __shfl_xor(q, 1, 64);
        if (t == 0 && g < groups) gn_mean_rstd(a, q, n, eps, &s_mean[g], &s_rstd[g]);
    }
    __syncthreads();
}
// the affine a normalised channel is written with: y = x * sc + sh
__device__ __forceinline__ void gn_coef(float gamma, float beta, float mean, float rstd, float& sc, float& sh) {
    const float w = gamma * rstd;
    sc = w;
    sh = beta - mean * w;
}

// one 16-byte vector into its channels' f32 partials
template <typename T>
__device__ __forceinline__ void gn_accum(const typename Vec16<T>::type& v, float (&s1)[Vec16<T>::N], float (&s2)[Vec16<T>::N]) {
#pragma unroll
    for (int e = 0; e < Vec16<T>::N; ++e) {
        const float f = (float)v[e];
        s1[e] += f;
        s2[e] = fmaf(f, f, s2[e]);
    }
}
// y = x * sc + sh [* sigmoid], rounded to T, one 16-byte store
template <typename T, bool SILU>
__device__ __forceinline__ void gn_out(const typename Vec16<T>::type& v, const float (&sc)[Vec16<T>::N], const float (&sh)[Vec16<T>::N],
                                       T* dst) {
    typename Vec16<T>::type o;
#pragma unroll
    for (int e = 0; e < Vec16<T>::N; ++e) {
        float y = fmaf((float)v[e], sc[e], sh[e]);
        if (SILU) y = silu_fast(y);
        o[e] = (T)y;
    }
    *reinterpret_cast<typename Vec16<T>::type*>(dst) = o;
}

// grid (chunks, B); NS = channel slots per thread, UNR = rows in flight per thread
template <typename T, int NS, int UNR>
__global__ __launch_bounds__(GN_THREADS) void gn_stats_kernel(const T* __restrict__ x0, int C0,
                                                              const T* __restrict__ x1, int C1, int HW,
                                                              int groups, double* __restrict__ part) {
    constexpr int VEC = Vec16<T>::N;
    typedef typename Vec16<T>::type V;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int C = C0 + C1, S = C / VEC;
    const int tpr = S < GN_THREADS ? S : GN_THREADS;          // threads per row
    const int R = GN_THREADS / tpr;                            // rows in flight
    const int tid = threadIdx.x;
    const int trow = tid / tpr, tcol = tid - trow * tpr;
    const int chunks = gridDim.x, chunk = blockIdx.x, b = blockIdx.y;
    const int r0 = (int)((long)HW * chunk / chunks), r1 = (int)((long)HW * (chunk + 1) / chunks);

    float s1[NS][VEC], s2[NS][VEC];
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
        for (int e = 0; e < VEC; ++e) s1[k][e] = s2[k][e] = 0.f;

    if (trow < R) {
        // UNR rows in flight per thread: all loads of a batch are issued before the first is consumed
        int r = r0 + trow;
        for (; r + (UNR - 1) * R < r1; r += UNR * R) {
            V v[UNR][NS];
#pragma unroll
            for (int u = 0; u < UNR; ++u)
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    const int slot = tcol + k * tpr;
                    if (slot < S) v[u][k] = load_slot<T>(x0, C0, x1, C1, (size_t)b * HW + r + u * R, slot * VEC);
                }
#pragma unroll
            for (int u = 0; u < UNR; ++u)
#pragma unroll
                for (int k = 0; k < NS; ++k)
                    if (tcol + k * tpr < S) gn_accum<T>(v[u][k], s1[k], s2[k]);
        }
        if constexpr (UNR > 1)      // (UNR = 1: the loop above takes every row)
        for (; r < r1; r += R) {
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int slot = tcol + k * tpr;
                if (slot < S) gn_accum<T>(load_slot<T>(x0, C0, x1, C1, (size_t)b * HW + r, slot * VEC), s1[k], s2[k]);
            }
        }
    }
    // per-channel partials of the R row lanes -> LDS [R][C][2]
    float* lds = reinterpret_cast<float*>(smem);
    if (trow < R) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int slot = tcol + k * tpr;
            if (slot < S) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    lds[((size_t)trow * C + slot * VEC + e) * 2 + 0] = s1[k][e];
                    lds[((size_t)trow * C + slot * VEC + e) * 2 + 1] = s2[k][e];
                }
            }
        }
    }
    __syncthreads();
    int gp2 = 1;
    while (gp2 < groups) gp2 *= 2;
    int g, t;
    double a, q;
    gn_group_fold<true>(lds, C, R, C / groups, groups, GN_THREADS / gp2, tid, g, t, a, q);     // >= 4 threads per group (groups <= 64)
    if (t == 0 && g < groups) {
        double* o = part + (((size_t)b * chunks + chunk) * groups + g) * 2;
        o[0] = a;
        o[1] = q;
    }
}

// Statistics from the producing conv's epilogue (gemm.hip, GemmArgs.gn_part): part32[b][chunk][quad][2] f32 = (sum, sum of squares) of
// one wave's 64 rows x one 4-channel quad, chunk = (256-row tile of the image) x 4 + wave row.  One workgroup per (group, image) folds
// them into out[b][0][g][2] (f64; the layout gn_apply_kernel reads with chunks = 1): thread t takes chunks t, t + 256, ... (the
// group's quads in order inside a chunk), then a fixed xor-shuffle tree per wave and the four waves in order.
__global__ __launch_bounds__(GN_THREADS) void gn_fold_kernel(const float* __restrict__ part32, int chunks, int quads, int groups,
                                                             double* __restrict__ out) {
    __shared__ double s_w[GN_THREADS / 64][2];
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int qpg = quads / groups;
    double a = 0.0, q = 0.0;
    const float* src = part32 + ((size_t)b * chunks * quads + (size_t)g * qpg) * 2;
    for (int c = tid; c < chunks; c += GN_THREADS)
        for (int k = 0; k < qpg; ++k) {
            const float2 pr = *reinterpret_cast<const float2*>(src + ((size_t)c * quads + k) * 2);
            a += (double)pr.x;
            q += (double)pr.y;
        }
    gn_pair_tree(a, q, 64);
    gn_pair_waves(s_w, tid, tid == 0, 0, GN_THREADS / 64, a, q);
    if (tid == 0) {
        out[((size_t)b * groups + g) * 2] = a;
        out[((size_t)b * groups + g) * 2 + 1] = q;
    }
}

// grid (row_blocks, B)
template <typename T, bool SILU, int NS, int UNR>
__global__ __launch_bounds__(GN_THREADS) void gn_apply_kernel(const T* __restrict__ x0, int C0,
                                                              const T* __restrict__ x1, int C1,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta,
                                                              T* __restrict__ out, int HW, int groups,
                                                              float eps, int chunks,
                                                              const double* __restrict__ part) {
    constexpr int VEC = Vec16<T>::N;
    typedef typename Vec16<T>::type V;
    __shared__ float s_mean[64], s_rstd[64];
    const int C = C0 + C1, S = C / VEC;
    const int tpr = S < GN_THREADS ? S : GN_THREADS;
    const int R = GN_THREADS / tpr;
    const int tid = threadIdx.x;
    const int trow = tid / tpr, tcol = tid - trow * tpr;
    const int b = blockIdx.y;
    const int cpg = C / groups;
    extern __shared__ __attribute__((aligned(16))) char smem_apply[];
    gn_fold_partials(part, b, chunks, groups, (double)HW * cpg, eps, reinterpret_cast<double*>(smem_apply), s_mean, s_rstd);
    if (trow >= R) return;
    float sc[NS][VEC], sh[NS][VEC];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int slot = tcol + k * tpr;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (slot < S) {
                const int c = slot * VEC + e, g = c / cpg;
                gn_coef(gamma[c], beta[c], s_mean[g], s_rstd[g], sc[k][e], sh[k][e]);
            } else {
                sc[k][e] = sh[k][e] = 0.f;
            }
        }
    }
    const int rows_per_block = (HW + gridDim.x - 1) / gridDim.x;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = (r0 + rows_per_block < HW) ? r0 + rows_per_block : HW;
    int r = r0 + trow;
    for (; r + (UNR - 1) * R < r1; r += UNR * R) {
        V v[UNR][NS];
#pragma unroll
        for (int u = 0; u < UNR; ++u)
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int slot = tcol + k * tpr;
                if (slot < S) v[u][k] = load_slot<T>(x0, C0, x1, C1, (size_t)b * HW + r + u * R, slot * VEC);
            }
#pragma unroll
        for (int u = 0; u < UNR; ++u)
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const int slot = tcol + k * tpr;
                if (slot < S) gn_out<T, SILU>(v[u][k], sc[k], sh[k], out + ((size_t)b * HW + r + u * R) * C + slot * VEC);
            }
    }
    if constexpr (UNR > 1)
    for (; r < r1; r += R) {
        const size_t row = (size_t)b * HW + r;
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int slot = tcol + k * tpr;
            if (slot < S) gn_out<T, SILU>(load_slot<T>(x0, C0, x1, C1, row, slot * VEC), sc[k], sh[k], out + row * C + slot * VEC);
        }
    }
}

// The statistics-only GroupNorm (launch_groupnorm_stats): after the statistics pass, gn_apply_kernel's fold and coefficients once per
// image into coef[b][2][C] f32 = (sc[c], sh[c]); the consumer (rowres.hip, gn_rowlin_kernel) applies y = fmaf(x, sc, sh) to the rows it
// holds.  grid (B).
__global__ __launch_bounds__(GN_THREADS) void gn_coef_kernel(const float* __restrict__ gamma, const float* __restrict__ beta, int C, int HW,
                                                             int groups, float eps, int chunks, const double* __restrict__ part,
                                                             float* __restrict__ coef) {
    __shared__ float s_mean[64], s_rstd[64];
    extern __shared__ __attribute__((aligned(16))) char smem_coef[];
    const int b = blockIdx.x, cpg = C / groups;
    gn_fold_partials(part, b, chunks, groups, (double)HW * cpg, eps, reinterpret_cast<double*>(smem_coef), s_mean, s_rstd);
    for (int c = threadIdx.x; c < C; c += GN_THREADS) {
        float sc, sh;
        gn_coef(gamma[c], beta[c], s_mean[c / cpg], s_rstd[c / cpg], sc, sh);
        coef[(size_t)b * 2 * C + c] = sc;
        coef[(size_t)b * 2 * C + C + c] = sh;
    }
}

// one wave per RPW consecutive rows (all RPW*MAXS loads of a wave are issued before any reduction, so narrow rows
// -- C = 320 fills only 40 of 64 lanes -- still keep enough bytes in flight); 4 waves per workgroup.
// MOD: no affine; y = xhat * (1 + scale[half][c]) + shift[half][c] with gamma = scale, beta = shift, [2][C] each
template <typename T, bool MOD, int MAXS, int RPW>
__global__ __launch_bounds__(256) void layernorm_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, T* __restrict__ out,
                                                        int M, int C, float eps, int rows_per_batch) {
    constexpr int VEC = Vec16<T>::N;        // C <= 64*MAXS*VEC
    typedef typename Vec16<T>::type V;
    const int lane = threadIdx.x & 63;
    const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW;
    if (row0 >= M) return;
    const int S = C / VEC;
    V t[RPW][MAXS];
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
        const int row = row0 + rr < M ? row0 + rr : M - 1;
#pragma unroll
        for (int k = 0; k < MAXS; ++k) {
            const int slot = lane + k * 64;
            if (slot < S) t[rr][k] = *reinterpret_cast<const V*>(x + (size_t)row * C + slot * VEC);
        }
    }
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
        const int row = row0 + rr;
        if (row >= M) break;
        float v[MAXS][VEC];
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < MAXS; ++k) {
            const int slot = lane + k * 64;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                v[k][e] = slot < S ? (float)t[rr][k][e] : 0.f;
                sum += v[k][e];
            }
        }
        const float mean = wave_sum(sum) / (float)C;
        float sq = 0.f;
#pragma unroll
        for (int k = 0; k < MAXS; ++k) {
            const int slot = lane + k * 64;
            if (slot < S) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) { const float d = v[k][e] - mean; sq = fmaf(d, d, sq); }
            }
        }
        const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)C + eps);
        T* orow = out + (size_t)row * C;
#pragma unroll
        for (int k = 0; k < MAXS; ++k) {
            const int slot = lane + k * 64;
            if (slot < S) {
                V o;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int c = slot * VEC + e;
                    if (MOD) {
                        const int hoff = ((row / rows_per_batch) & 1) * C;
                        o[e] = (T)fmaf((v[k][e] - mean) * rstd, 1.0f + gamma[hoff + c], beta[hoff + c]);
                    } else {
                        o[e] = (T)fmaf((v[k][e] - mean) * rstd, gamma[c], beta[c]);
                    }
                }
                *reinterpret_cast<V*>(orow + slot * VEC) = o;
            }
        }
    }
}

// Affine LayerNorm with LPR lanes per row (LPR = the largest power of two dividing the row's S 16-byte chunks, CPL = S / LPR
// chunks per lane): a wave pass covers 64 / LPR rows with all 64 lanes busy, lane s of a row owning chunks s, s + LPR, ... so
// every load instruction reads runs of LPR * 16 contiguous bytes.  C = 320 (40 chunks) keeps 8 lanes x 5 chunks per row
// instead of 40 of 64 lanes and a six-step cross-lane reduction per row: 2.4x fewer VALU instructions per byte, which is
// what bounded the wave-per-row form at the 64 x 64 level.  gamma / beta sit in LDS; the next pass's rows are in flight
// while the current pass is reduced.  Two-pass statistics (mean, then centred squares), fixed order per shape.
template <typename T, int CPL>
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, T* __restrict__ out,
                                                             int M, int C, float eps, int LPR, int passes) {
    constexpr int VEC = Vec16<T>::N;
    typedef typename Vec16<T>::type V;
    extern __shared__ __attribute__((aligned(16))) char smem_ln[];
    float* s_g = reinterpret_cast<float*>(smem_ln);
    float* s_b = s_g + C;
    for (int i = threadIdx.x; i < C; i += 256) { s_g[i] = gamma[i]; s_b[i] = beta[i]; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rpw = 64 / LPR;                                  // rows per wave pass
    const int sub = lane & (LPR - 1), rl = lane / LPR;
    const int base = (blockIdx.x * 4 + wave) * passes * rpw;
    if (base >= M) return;
    const float invC = 1.0f / (float)C;
    V t[CPL], tn[CPL];
    {
        const int row = base + rl < M ? base + rl : M - 1;
#pragma unroll
        for (int k = 0; k < CPL; ++k) t[k] = *reinterpret_cast<const V*>(x + (size_t)row * C + (sub + LPR * k) * VEC);
    }
    for (int p = 0; p < passes; ++p) {
        const int row = base + p * rpw + rl;
        if (base + p * rpw >= M) break;                        // wave-uniform
        if (p + 1 < passes) {
            const int nr = row + rpw < M ? row + rpw : M - 1;
#pragma unroll
            for (int k = 0; k < CPL; ++k) tn[k] = *reinterpret_cast<const V*>(x + (size_t)nr * C + (sub + LPR * k) * VEC);
        }
        float v[CPL][VEC];
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k)
#pragma unroll
            for (int e = 0; e < VEC; ++e) { v[k][e] = (float)t[k][e]; sum += v[k][e]; }
        const float mean = lpr_sum(sum, LPR) * invC;
        float sq = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k)
#pragma unroll
            for (int e = 0; e < VEC; ++e) { v[k][e] -= mean; sq = fmaf(v[k][e], v[k][e], sq); }
        const float rstd = 1.0f / sqrtf(lpr_sum(sq, LPR) * invC + eps);
        if (row < M) {
            T* orow = out + (size_t)row * C;
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                const int c = (sub + LPR * k) * VEC;
                V o;
#pragma unroll
                for (int e = 0; e < VEC; ++e) o[e] = (T)fmaf(v[k][e] * rstd, s_g[c + e], s_b[c + e]);
                *reinterpret_cast<V*>(orow + c) = o;
            }
        }
#pragma unroll
        for (int k = 0; k < CPL; ++k) t[k] = tn[k];
    }
}

// softmax over rows of `cols` elements (one 256-thread workgroup per row; cols % VEC == 0).  Used by
// the VAE encoder's single-head 512-d mid-block attention, whose score matrix is materialised by
// the GEMM kernel.
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const T* __restrict__ x, T* __restrict__ out, int cols,
                                                           float scale_log2) {
    constexpr int VEC = Vec16<T>::N;
    typedef typename Vec16<T>::type V;
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const T* xr = x + (size_t)blockIdx.x * cols;
    T* orow = out + (size_t)blockIdx.x * cols;
    const int S = cols / VEC;
    float m = -INFINITY;
    for (int s = tid; s < S; s += 256) {
        const V v = *reinterpret_cast<const V*>(xr + s * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) m = fmaxf(m, (float)v[e]);
    }
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float mb = m * scale_log2;
    float sum = 0.f;
    for (int s = tid; s < S; s += 256) {
        const V v = *reinterpret_cast<const V*>(xr + s * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) sum += exp2f(fmaf((float)v[e], scale_log2, -mb));
    }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float inv = 1.0f / ((red[4] + red[5]) + (red[6] + red[7]));
    for (int s = tid; s < S; s += 256) {
        const V v = *reinterpret_cast<const V*>(xr + s * VEC);
        V o;
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = (T)(exp2f(fmaf((float)v[e], scale_log2, -mb)) * inv);
        *reinterpret_cast<V*>(orow + s * VEC) = o;
    }
}

// One-pass GroupNorm for the low-resolution levels (16 x 16 and 8 x 8 maps: 52 of the 83 GroupNorm launches of an SD1.5
// forward, 35 % of their time): a workgroup takes ALL HW rows of a channel slab made of whole groups of one image and keeps
// them in registers (<= MAXCH 16-byte chunks per thread), so the tensor is read once instead of twice and one launch
// replaces two.  grid (P slabs, B); a thread owns one chunk column and every R-th row, exactly like the two-pass kernels,
// and the statistics use the same per-channel f32 partials -> fixed-order f64 fold per group (bit-reproducible,
// independent of the batch size).
// STATS: the statistics alone -- the group's pair goes to part[b][0][g][2] (the scratch layout with chunks = 1) and nothing is written.
template <typename T, bool SILU, int MAXCH, bool STATS = false>
__global__ __launch_bounds__(GN_THREADS) void gn_onepass_kernel(const T* __restrict__ x0, int C0, const T* __restrict__ x1,
                                                                int C1, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, T* __restrict__ out, int HW,
                                                                int groups, float eps, int CS) {
    constexpr int VEC = Vec16<T>::N;
    typedef typename Vec16<T>::type V;
    extern __shared__ __attribute__((aligned(16))) char smem_op[];
    __shared__ float s_mean[64], s_rstd[64];
    const int C = C0 + C1, cpg = C / groups;
    const int tpr = CS / VEC;                                  // threads per row (chunk columns of the slab)
    const int R = GN_THREADS / tpr;                            // rows in flight
    const int tid = threadIdx.x, trow = tid / tpr, tcol = tid - trow * tpr;
    const int b = blockIdx.y, c0 = blockIdx.x * CS;            // first channel of this slab
    const int ch = c0 + tcol * VEC;                            // first channel of this thread's chunks
    const bool live = trow < R;
    V v[MAXCH];
    float s1[VEC], s2[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) s1[e] = s2[e] = 0.f;
    if (live) {
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            const int r = trow + i * R;
            if (r < HW) v[i] = load_slot<T>(x0, C0, x1, C1, (size_t)b * HW + r, ch);
        }
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            const int r = trow + i * R;
            if (r < HW) gn_accum<T>(v[i], s1, s2);
        }
    }
    float* lds = reinterpret_cast<float*>(smem_op);            // [R][CS][2]
    if (live) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            lds[((size_t)trow * CS + tcol * VEC + e) * 2 + 0] = s1[e];
            lds[((size_t)trow * CS + tcol * VEC + e) * 2 + 1] = s2[e];
        }
    }
    __syncthreads();
    const int gslab = CS / cpg;                                // whole groups in this slab (a power of two)
    int g, t;
    double a, q;
    gn_group_fold<false>(lds, CS, R, cpg, gslab, GN_THREADS / gslab, tid, g, t, a, q);          // 8 .. 256 threads per group
    if constexpr (STATS) {
        if (t == 0) {
            double* o = reinterpret_cast<double*>(out) + ((size_t)b * groups + c0 / cpg + g) * 2;
            o[0] = a;
            o[1] = q;
        }
        return;
    }
    if (t == 0) gn_mean_rstd(a, q, (double)HW * cpg, eps, &s_mean[g], &s_rstd[g]);
    __syncthreads();
    if (!live) return;
    float sc[VEC], sh[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const int c = ch + e, cg = (c - c0) / cpg;
        gn_coef(gamma[c], beta[c], s_mean[cg], s_rstd[cg], sc[e], sh[e]);
    }
#pragma unroll
    for (int i = 0; i < MAXCH; ++i) {
        const int r = trow + i * R;
        if (r < HW) gn_out<T, SILU>(v[i], sc, sh, out + ((size_t)b * HW + r) * C + ch);
    }
}

// ---- host side: one launch helper, one table per kernel family, one plan per operator.
// Every kernel of this file runs 256 threads.  A pointer argument is cast to the kernel's parameter type (void* -> T*); any other
// argument must already have it.
static_assert(GN_THREADS == 256, "the LayerNorm and softmax kernels index with 256 threads");
template <typename P, typename A>
P kernel_arg(A a) {
    if constexpr (std::is_pointer<P>::value) {
        return static_cast<P>(a);
    } else {
        static_assert(std::is_same<P, A>::value, "scalar kernel arguments are passed in the parameter's own type");
        return a;
    }
}
template <typename... P, typename... A>
int launch(void (*kern)(P...), dim3 grid, size_t lds, hipStream_t s, A... args) {
    hipLaunchKernelGGL(kern, grid, dim3(GN_THREADS), lds, s, kernel_arg<P>(args)...);
    DSIM_HIP_CHECK(hipGetLastError());
    return DSIM_OK;
}

// The compiled kernels, each instantiation named once; the plans choose a row and the launchers start that row, so a plan
// outside a table is DSIM_ERR_INVALID.  [2]: without / with SiLU (GroupNorm), affine / modulated (LayerNorm).
template <typename T> struct GnTwoPass {
    int NS, UNR;                                                // a thread's channel slots, and its rows in flight
    decltype(&gn_stats_kernel<T, 1, 1>) stats;
    decltype(&gn_apply_kernel<T, false, 1, 1>) apply[2];
};
template <typename T, int NS, int UNR>
constexpr GnTwoPass<T> gn_two_pass() {
    return {NS, UNR, gn_stats_kernel<T, NS, UNR>, {gn_apply_kernel<T, false, NS, UNR>, gn_apply_kernel<T, true, NS, UNR>}};
}
template <typename T> constexpr GnTwoPass<T> kGnTwoPass[] = {gn_two_pass<T, 1, 4>(), gn_two_pass<T, 2, 2>(), gn_two_pass<T, GN_MAX_SLOTS, 1>()};

constexpr int GN_OP_MAXCH = 24;
template <typename T> constexpr decltype(&gn_onepass_kernel<T, false, GN_OP_MAXCH>) kGnOnePass[2] = {
    gn_onepass_kernel<T, false, GN_OP_MAXCH>, gn_onepass_kernel<T, true, GN_OP_MAXCH>};
template <typename T> constexpr decltype(&gn_onepass_kernel<T, false, GN_OP_MAXCH>) kGnOnePassStats = gn_onepass_kernel<T, false, GN_OP_MAXCH, true>;

template <typename T> struct LnRows {
    int CPL;
    decltype(&layernorm_rows_kernel<T, 1>) kern;
};
template <typename T> constexpr LnRows<T> kLnRows[] = {{1, layernorm_rows_kernel<T, 1>}, {3, layernorm_rows_kernel<T, 3>}, {5, layernorm_rows_kernel<T, 5>}};

template <typename T> struct LnWave {
    int MAXS, RPW;                                              // rows up to 64 * MAXS chunks, RPW of them per wave
    decltype(&layernorm_kernel<T, false, 1, 1>) kern[2];
};
template <typename T, int MAXS, int RPW>
constexpr LnWave<T> ln_wave() { return {MAXS, RPW, {layernorm_kernel<T, false, MAXS, RPW>, layernorm_kernel<T, true, MAXS, RPW>}}; }
template <typename T> constexpr LnWave<T> kLnWave[] = {ln_wave<T, 1, 8>(), ln_wave<T, 2, 2>(), ln_wave<T, 3, 2>(), ln_wave<T, 6, 1>()};

// The LayerNorm dispatch, decided in one place: ln_typed launches what this returns and layernorm_plan() reports it.
//   form 0, layernorm_rows_kernel<T, CPL>: affine only, S = C / VEC <= 80 chunks with S / LPR (LPR = the largest power of two
//           dividing S, at most 64) a CPL of kLnRows; rows per workgroup = 4 waves x passes x (64 / LPR);
//   form 1, layernorm_kernel<T, MOD, MAXS, RPW>: every other width, on the narrowest row of kLnWave; rows per workgroup = 4 x RPW.
struct LnLaunch {
    dsim_ln_plan p;
    int row;                    // of kLnRows (form 0) / kLnWave (form 1)
    size_t lds;
};
template <typename T>
int ln_plan(int M, int C, bool mod, LnLaunch* l) {
    constexpr int VEC = Vec16<T>::N;
    if (C < VEC || C % VEC || C > 64 * 6 * VEC || M < 1) return DSIM_ERR_INVALID;
    const int S = C / VEC;
    *l = LnLaunch{};
    dsim_ln_plan* p = &l->p;
    if (!mod && S <= 80) {      // wider rows: the wave-per-row form below already streams at > 6 TB/s
        int LPR = 1;
        while (LPR < 64 && S % (LPR * 2) == 0) LPR *= 2;
        const int CPL = S / LPR;                       // odd by construction
        for (const LnRows<T>& k : kLnRows<T>) {
            if (k.CPL != CPL) continue;
            l->row = (int)(&k - kLnRows<T>);
            const int rpw = 64 / LPR;
            int passes = 4;                                             // rows per workgroup = 4 waves x passes x rpw
            while (passes > 1 && (M + 4 * passes * rpw - 1) / (4 * passes * rpw) < 2048) passes >>= 1;
            p->form = 0; p->LPR = LPR; p->CPL = CPL; p->passes = passes;
            p->blocks = (M + 4 * passes * rpw - 1) / (4 * passes * rpw);
            l->lds = (size_t)2 * C * sizeof(float);                     // gamma and beta
            return DSIM_OK;
        }
    }
    for (const LnWave<T>& k : kLnWave<T>) {
        if (S > 64 * k.MAXS) continue;
        l->row = (int)(&k - kLnWave<T>);
        p->form = 1; p->MAXS = k.MAXS; p->RPW = k.RPW;
        p->blocks = (M + 4 * k.RPW - 1) / (4 * k.RPW);
        return DSIM_OK;
    }
    return DSIM_ERR_INVALID;
}

template <typename T, bool MOD>
int ln_typed(const void* x, const float* gamma, const float* beta, void* out, int M, int C, float eps, int rpb,
             hipStream_t s) {
    LnLaunch l;
    if (ln_plan<T>(M, C, MOD, &l) != DSIM_OK) return DSIM_ERR_INVALID;
    const dsim_ln_plan& p = l.p;
    if (p.form == 0) return launch(kLnRows<T>[l.row].kern, dim3(p.blocks), l.lds, s, x, gamma, beta, out, M, C, eps, p.LPR, p.passes);
    return launch(kLnWave<T>[l.row].kern[MOD], dim3(p.blocks), l.lds, s, x, gamma, beta, out, M, C, eps, rpb);
}

// slab width (channels) of the one-pass form for this shape, or 0 when it does not apply: whole groups, 16-byte chunk
// columns of at least 256 B per row, no slab straddling the two concat sources, at most MAXCH chunks per thread
template <typename T>
int gn_onepass_slab(int C0, int C1, int HW, int groups) {
    constexpr int VEC = Vec16<T>::N;
    const int C = C0 + C1, cpg = C / groups;
    // The choice depends on the SHAPE only, never on the batch (which is why no batch size is passed): slab width sets the summation
    // grouping, and a batch of N must score bit for bit like N single images.  Widest legal slab = longest coalesced row segments
    // (narrower slabs with more, shorter workgroups measured slower at the 8 x 8 level: 17.7 vs 16.8 us, 29 vs 22 us at 2560 channels).
    int best = 0;
    for (int gs = 1; gs <= groups; gs *= 2) {                  // groups per slab
        const int CS = gs * cpg;
        if (groups % gs || CS % VEC || CS / VEC > GN_THREADS) continue;
        if (CS * (int)sizeof(T) < 256) continue;               // row segments shorter than 256 B waste the memory pipe
        if (C1 && (C0 % CS)) continue;                         // a slab may not straddle the concat boundary
        if (C / CS < 2) continue;                              // at least two workgroups per image
        const int tpr = CS / VEC, R = GN_THREADS / tpr;
        if ((HW + R - 1) / R > GN_OP_MAXCH) continue;
        if ((size_t)R * CS * 2 * sizeof(float) > 48 * 1024) continue;
        best = CS;
    }
    return best;
}

// The GroupNorm dispatch, decided in one place: gn_typed launches what this returns and groupnorm_plan() reports it.
//   form 0, one launch of gn_onepass_kernel: slab width CS (gn_onepass_slab), tpr = CS / VEC threads per row, R rows in flight;
//   form 1, gn_stats_kernel + gn_apply_kernel<NS, UNR> (the row of kGnTwoPass with room for the slots a thread owns): `chunks`
//           statistic slabs and rb apply row blocks per image;
//   form 2, gn_fold_kernel + gn_apply_kernel: the statistics come from a conv epilogue (chunks = 1: the folded pair).
// grid / lds: the first launch (one-pass, statistics or fold); agrid / alds: the apply pass of forms 1 and 2.
struct GnLaunch {
    dsim_gn_plan p;
    int row;                    // of kGnTwoPass (forms 1 and 2)
    dim3 grid, agrid;
    size_t lds, alds;
};
template <typename T>
int gn_plan(int C0, int C1, int B, int HW, int groups, bool pre, GnLaunch* l) {
    constexpr int VEC = Vec16<T>::N;
    const int C = C0 + C1;
    if (B < 1 || HW < 1 || groups < 1 || C < VEC) return DSIM_ERR_INVALID;
    if (C % groups || C0 % VEC || C1 % VEC || groups > 64 || C > GN_MAX_SLOTS * GN_THREADS * VEC)
        return DSIM_ERR_INVALID;
    // (precomputed statistics: whole 4-channel quads per group)
    if (pre && (C1 || (C / groups) % 4)) return DSIM_ERR_INVALID;
    *l = GnLaunch{};
    dsim_gn_plan* p = &l->p;
    if (const int CS = !pre ? gn_onepass_slab<T>(C0, C1, HW, groups) : 0) {
        p->form = 0; p->NS = 1; p->CS = CS; p->tpr = CS / VEC; p->R = GN_THREADS / p->tpr;
        l->grid = dim3(C / CS, B);
        l->lds = (size_t)p->R * CS * 2 * sizeof(float);
        return DSIM_OK;
    }
    const int S = C / VEC, tpr = S < GN_THREADS ? S : GN_THREADS, R = GN_THREADS / tpr;
    if ((size_t)R * C * 2 * sizeof(float) > 64 * 1024) return DSIM_ERR_INVALID;      // gn_stats_kernel's LDS
    // row blocks per image of the apply pass (no effect on the numbers): about 1024 workgroups in all, so that large
    // batches amortise each workgroup's statistics fold over more rows and small batches still fill the chip
    int rb = HW / (R * 4);
    const int want = (1024 + B - 1) / B;
    if (rb > want) rb = want;
    rb = rb < 1 ? 1 : (rb > 64 ? 64 : rb);
    const int ns = (S + tpr - 1) / tpr;
    for (const GnTwoPass<T>& k : kGnTwoPass<T>) {
        if (k.NS < ns) continue;
        l->row = (int)(&k - kGnTwoPass<T>);
        p->form = pre ? 2 : 1;
        p->NS = k.NS; p->UNR = k.UNR;
        p->CS = C; p->tpr = tpr; p->R = R;
        p->chunks = pre ? 1 : gn_chunks(HW);
        p->rb = rb;
        l->grid = pre ? dim3(groups, B) : dim3(p->chunks, B);
        l->lds = pre ? 0 : (size_t)R * C * 2 * sizeof(float);
        l->agrid = dim3(rb, B);
        l->alds = (size_t)p->chunks * groups * 2 * sizeof(double);      // <= 32 KB
        return DSIM_OK;
    }
    return DSIM_ERR_INVALID;
}

// pre: the statistics pass already happened in the producing conv's epilogue (GemmArgs.gn_part): gn_fold_kernel folds its
// per-(wave, 4-channel quad) f32 partials into one f64 pair per (image, group), in fixed order
template <typename T>
int gn_typed(const void* x0, int C0, const void* x1, int C1, const float* gamma, const float* beta,
             void* out, int B, int HW, int groups, float eps, int silu, void* scratch, hipStream_t s,
             const float* pre = nullptr, int pre_chunks = 0) {
    if (!x1) C1 = 0;
    GnLaunch l;
    if (gn_plan<T>(C0, C1, B, HW, groups, pre != nullptr, &l) != DSIM_OK) return DSIM_ERR_INVALID;
    const dsim_gn_plan& p = l.p;
    const int si = silu ? 1 : 0;
    if (p.form == 0) return launch(kGnOnePass<T>[si], l.grid, l.lds, s, x0, C0, x1, C1, gamma, beta, out, HW, groups, eps, p.CS);
    const GnTwoPass<T>& k = kGnTwoPass<T>[l.row];
    const int st = p.form == 2 ? launch(gn_fold_kernel, l.grid, l.lds, s, pre, pre_chunks, (C0 + C1) / 4, groups, scratch)
                               : launch(k.stats, l.grid, l.lds, s, x0, C0, x1, C1, HW, groups, scratch);
    if (st != DSIM_OK) return st;
    return launch(k.apply[si], l.agrid, l.alds, s, x0, C0, x1, C1, gamma, beta, out, HW, groups, eps, p.chunks, scratch);
}

// The statistics-only GroupNorm: the statistics of the form launch_groupnorm takes for this shape (the one-pass form's own f32 partials
// and fold where it applies, else gn_stats_kernel) into the scratch, then gn_coef_kernel into the caller's table coef [B][2][C].
template <typename T>
int gn_stats_typed(const void* x, int C, const float* gamma, const float* beta, int B, int HW, int groups, float eps, void* scratch,
                   float* coef, hipStream_t s) {
    GnLaunch l;
    if (gn_plan<T>(C, 0, B, HW, groups, false, &l) != DSIM_OK) return DSIM_ERR_INVALID;
    const dsim_gn_plan& p = l.p;
    const int chunks = p.form == 0 ? 1 : p.chunks;
    // (the one-pass statistics kernel writes its pairs through `out`)
    const int st = p.form == 0 ? launch(kGnOnePassStats<T>, l.grid, l.lds, s, x, C, (const void*)nullptr, 0, gamma, beta, scratch, HW, groups, eps, p.CS)
                               : launch(kGnTwoPass<T>[l.row].stats, l.grid, l.lds, s, x, C, (const void*)nullptr, 0, HW, groups, scratch);
    if (st != DSIM_OK) return st;
    return launch(gn_coef_kernel, dim3(B), (size_t)chunks * groups * 2 * sizeof(double), s, gamma, beta, C, HW, groups, eps, chunks, scratch, coef);
}

}  // namespace

// the kernels launch_groupnorm (pre = 0) / launch_groupnorm_pre (pre = 1) start for this shape; host only
int groupnorm_plan(int C0, int C1, int B, int HW, int groups, int dtype, int pre, dsim_gn_plan* p) {
    if (!p || (dtype != DSIM_F32 && dtype != DSIM_BF16 && dtype != DSIM_F16) || (dtype == DSIM_F32 && pre)) return DSIM_ERR_INVALID;
    GnLaunch l;
    if ((dtype == DSIM_F32 ? gn_plan<float>(C0, C1, B, HW, groups, false, &l)
                           : gn_plan<bf16_t>(C0, C1, B, HW, groups, pre != 0, &l)) != DSIM_OK) return DSIM_ERR_INVALID;    // (bf16_t: either 16-bit type)
    *p = l.p;
    return DSIM_OK;
}

// the kernel launch_layernorm (mod = 0) / launch_layernorm_mod (mod = 1) starts for this shape; host only
int layernorm_plan(int M, int C, int dtype, int mod, dsim_ln_plan* p) {
    if (!p || (dtype != DSIM_F32 && dtype != DSIM_BF16 && dtype != DSIM_F16)) return DSIM_ERR_INVALID;
    LnLaunch l;
    if ((dtype == DSIM_F32 ? ln_plan<float>(M, C, mod != 0, &l) : ln_plan<bf16_t>(M, C, mod != 0, &l)) != DSIM_OK) return DSIM_ERR_INVALID;
    *p = l.p;                                                       // (bf16_t: either 16-bit type)
    return DSIM_OK;
}

// passes over the tensor the GroupNorm of this shape makes (2 = one-pass form: read + write; 3 = statistics read + read + write)
int groupnorm_passes(int C0, int C1, int HW, int groups, int dtype) {
    dsim_gn_plan p;
    if (groupnorm_plan(C0, C1, 1, HW, groups, dtype, 0, &p) != DSIM_OK) return 3;
    return p.form == 0 ? 2 : 3;
}

size_t groupnorm_scratch_bytes(int B, int groups) { return (size_t)B * 64 * groups * 2 * sizeof(double); }

// GroupNorm(+SiLU) whose statistics pass already ran in the producing conv's epilogue: part32 = GemmArgs.gn_part of that launch,
// chunks = its partial rows per image (HW / 64); 16-bit dtypes only
int launch_groupnorm_pre(const void* x, int C, const float* gamma, const float* beta, void* out, int B, int HW, int groups, float eps,
                         int silu, int dtype, void* scratch, const float* part32, int chunks, hipStream_t s) {
    if (!part32 || chunks < 1 || dtype == DSIM_F32) return DSIM_ERR_INVALID;
    return by_dtype(dtype, [&](auto e) {
        return gn_typed<typename decltype(e)::type>(x, C, nullptr, 0, gamma, beta, out, B, HW, groups, eps, silu, scratch, s, part32, chunks);
    });
}

int launch_groupnorm(const void* x0, int C0, const void* x1, int C1, const float* gamma, const float* beta,
                     void* out, int B, int HW, int groups, float eps, int silu, int dtype, void* scratch,
                     hipStream_t s) {
    return by_dtype(dtype, [&](auto e) {
        return gn_typed<typename decltype(e)::type>(x0, C0, x1, C1, gamma, beta, out, B, HW, groups, eps, silu, scratch, s);
    });
}

int launch_groupnorm_stats(const void* x, int C, const float* gamma, const float* beta, int B, int HW, int groups, float eps, int dtype,
                           void* scratch, float* coef, hipStream_t s) {
    if (!coef || dtype == DSIM_F32) return DSIM_ERR_INVALID;
    return by_dtype(dtype, [&](auto e) { return gn_stats_typed<typename decltype(e)::type>(x, C, gamma, beta, B, HW, groups, eps, scratch, coef, s); });
}

int launch_layernorm(const void* x, const float* gamma, const float* beta, void* out, int M, int C, float eps,
                     int dtype, hipStream_t s) {
    return by_dtype(dtype, [&](auto e) { return ln_typed<typename decltype(e)::type, false>(x, gamma, beta, out, M, C, eps, 1, s); });
}

int launch_layernorm_mod(const void* x, const float* scale2, const float* shift2, void* out, int M, int C,
                         int rows_per_batch, float eps, int dtype, hipStream_t s) {
    if (rows_per_batch < 1) return DSIM_ERR_INVALID;
    return by_dtype(dtype, [&](auto e) {
        return ln_typed<typename decltype(e)::type, true>(x, scale2, shift2, out, M, C, eps, rows_per_batch, s);
    });
}

int launch_softmax_rows(const void* x, void* out, int rows, int cols, float scale, int dtype, hipStream_t s) {
    return by_dtype(dtype, [&](auto e) {
        typedef typename decltype(e)::type T;
        if (cols % Vec16<T>::N || rows < 1) return (int)DSIM_ERR_INVALID;
        return launch(softmax_rows_kernel<T>, dim3(rows), 0, s, x, out, cols, scale * 1.4426950408889634f);
    });
}

}  // namespace dsim
