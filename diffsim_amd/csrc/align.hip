// Token alignments: the cross-attention the DiffSim score is built on, returned instead of consumed.  The score tail (tails.hip) is
// cross-attention of image A's queries over image B's keys -- diffsim/diffsim.py:177-180 of the reference -- and its fused kernels use
// softmax(Q_a K_b^T / sqrt(D)) in registers and drop it; these kernels compute that matrix for its own sake.  They share the tiled
// core's fragments, MFMA wrappers, K tile geometry and head-dim dispatch (attn_core.h), but not attend: there is no V and no O.
#include "attn_core.h"

namespace dsim {
namespace {

// For direction a->b, P_bh[i][j] = softmax_j(Q_a[b,h,i,:] . K_b[b,h,j,:] / sqrt(D)) and Pm = mean of P_bh over the B CFG halves
// and the H heads; per query token i the kernels return argmax_j Pm[i][j] (ties: lowest j), its weight, the soft-argmax position
// sum_j Pm[i][j] (row_j, col_j) on the other image's grid, and on request Pm.
//
// The logits come from UN-RESCALED Q: S^T = K Q^T on the MFMAs from the stored values (accumulators start at 0), and the scale
// enters in f32 afterwards, P = exp2(fma(s, c, -m c)) with c = log2(e) / sqrt(D), as attn_short_kernel does.  Nothing is rounded to
// 16 bits between the inputs and Pm.  The score tail's attend pre-scales Q and rounds it to the compute dtype (load_q), so its
// probabilities differ from these in the last bits.
//
// Two passes, one logit routine (align_logits, attn_core.h: both take s from the same MFMA sequence on the same operands):
//   align_stats_kernel  one workgroup per (query tile, b h, pair, direction): the row's final maximum m and denominator
//                       l = sum_j exp2(fma(s, c, -m c)) (online over the key tiles), stored as (-m c, 1 / l): the workspace,
//                       [pair][dir][bh][N] float2, is all that reaches HBM besides the outputs;
//   align_kernel        one workgroup per (query tile, pair, direction): per 64-key tile, Pm = (sum over (b, h) ascending of
//                       exp2(fma(s, c, -m c)) / l) / (B H), then the finished tile is folded into the lane's running best, its
//                       index and the two coordinate sums (and stored, if attn is asked for).
// A probability depends on its key row only through s, so bit-identical key rows give bit-identical columns of Pm, whichever tile
// or block they fall in.  No atomics: every output element has one writer; status is a plain store of 1 by any row that saw a
// non-finite probability, into a word the launcher zeroed.
// this thread's chunks of a K tile on their way from global memory to LDS
template <typename T, int D> struct AlignRegs {
    static constexpr int CPRD = D / ACfg<T, D>::VEC;                 // real 16-B chunks per K row
    static constexpr int N = (KT * CPRD + 255) / 256;
    u32x4 k[N];
};

// the D real columns of key rows kv0 .. kv0 + 63 (those < Nk) of one (image, b, h): global -> registers, registers -> the LDS tile
// (ACfg's K row stride; the padding columns and the never-stored rows keep the zeros of align_zero_tile or stale finite values
// whose logits are masked)
template <typename T, int D>
__device__ __forceinline__ void align_k_load(AlignRegs<T, D>& sr, const T* kb, int ldk, int kv0, int Nk, int tid) {
    typedef AlignRegs<T, D> SR;
#pragma unroll
    for (int i = 0; i < SR::N; ++i) {
        const int idx = tid + i * 256, r = idx / SR::CPRD, c = idx - r * SR::CPRD;
        if (idx < KT * SR::CPRD && kv0 + r < Nk)
            sr.k[i] = *reinterpret_cast<const u32x4*>(kb + (size_t)(kv0 + r) * ldk + c * ACfg<T, D>::VEC);
    }
}
template <typename T, int D>
__device__ __forceinline__ void align_k_store(char* lds, const AlignRegs<T, D>& sr, int kv0, int Nk, int tid) {
    typedef AlignRegs<T, D> SR;
#pragma unroll
    for (int i = 0; i < SR::N; ++i) {
        const int idx = tid + i * 256, r = idx / SR::CPRD, c = idx - r * SR::CPRD;
        if (idx < KT * SR::CPRD && kv0 + r < Nk) *reinterpret_cast<u32x4*>(lds + r * ACfg<T, D>::RS + c * 16) = sr.k[i];
    }
}
template <typename T, int D>
__device__ __forceinline__ void align_zero_tile(char* lds, int tid) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (int o = tid * 16; o < ACfg<T, D>::TILEK; o += 256 * 16) *reinterpret_cast<u32x4*>(lds + o) = z;
}

// pass 1.  grid (ceil(N/128), B*H, n_pairs*2)
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void align_stats_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                             const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_b, int B,
                                                             int H, int N, float c, float2* __restrict__ stats) {
    typedef ACfg<T, D> C;
    __shared__ __attribute__((aligned(16))) char lds[C::TILEK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
    const int pair = blockIdx.z >> 1, dir = blockIdx.z & 1;
    const int ia = idx_a[pair], ib = idx_b[pair];
    const int iq = dir ? ib : ia, ix = dir ? ia : ib;
    const int ld = H * D;
    const size_t img = (size_t)B * N * ld, boff = (size_t)b * N * ld + h * D;
    const int q = blockIdx.x * 128 + wave * 32 + l31, qc = q < N ? q : N - 1;
    QFrags<T, D> qf;
    align_load_q<T, D>(qf, qg + iq * img + boff + (size_t)qc * ld, half);
    const T* kb = kg + ix * img + boff;
    const int ntiles = (N + KT - 1) / KT;
    AlignRegs<T, D> sr;
    align_k_load<T, D>(sr, kb, ld, 0, N, tid);
    align_zero_tile<T, D>(lds, tid);
    float mc = INFINITY, l = 0.f;          // -m c of the running maximum m (none yet); this half's share of the denominator
    for (int kt = 0; kt < ntiles; ++kt) {
        __syncthreads();                   // the tile is zeroed / the previous tile's fragments are read
        align_k_store<T, D>(lds, sr, kt * KT, N, tid);
        __syncthreads();
        if (kt + 1 < ntiles) align_k_load<T, D>(sr, kb, ld, (kt + 1) * KT, N, tid);
        f32x16 s[2];
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) s[jb] = align_logits<T, D>(qf, lds, jb, l31, half);
        float tmax = -INFINITY;
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (kt * KT + align_key(jb, r, half) >= N) s[jb][r] = -INFINITY;
                tmax = fmaxf(tmax, s[jb][r]);
            }
        tmax = max_halves(tmax);
        const float mc_new = fminf(mc, -tmax * c);
        const float alpha = __builtin_amdgcn_exp2f(mc_new - mc);        // tile 0: exp2(-inf) = 0 against l = 0
        mc = mc_new;
        float psum = 0.f;
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) psum += __builtin_amdgcn_exp2f(fmaf(s[jb][r], c, mc));
        l = fmaf(l, alpha, psum);
    }
    l = half_sum(l);
    if (half == 0 && q < N) stats[((size_t)blockIdx.z * gridDim.y + bh) * N + q] = make_float2(mc, 1.0f / l);
}

// pass 2.  grid (ceil(N/128), n_pairs*2)
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void align_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                       const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_b, int B, int H,
                                                       int N, float c, float rbh, int grid_w, const float2* __restrict__ stats,
                                                       int32_t* __restrict__ match, float* __restrict__ weight, float* __restrict__ expect,
                                                       float* __restrict__ attn, int32_t* __restrict__ status) {
    typedef ACfg<T, D> C;
    __shared__ __attribute__((aligned(16))) char lds[C::TILEK];
    __shared__ float2 pos[KT];             // (row, col) of the tile's keys on the other image's grid; (0, 0) past the end
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int pd = blockIdx.y, pair = pd >> 1, dir = pd & 1;
    const int ia = idx_a[pair], ib = idx_b[pair];
    const int iq = dir ? ib : ia, ix = dir ? ia : ib;
    const int BH = B * H, ld = H * D;
    const size_t img = (size_t)B * N * ld;
    const int q = blockIdx.x * 128 + wave * 32 + l31, qc = q < N ? q : N - 1;
    const T* qrow = qg + iq * img + (size_t)qc * ld;
    const T* kimg = kg + ix * img;
    const float2* st = stats + (size_t)pd * BH * N + qc;
    const int ntiles = (N + KT - 1) / KT;
    AlignRegs<T, D> sr;
    align_k_load<T, D>(sr, kimg, ld, 0, N, tid);
    align_zero_tile<T, D>(lds, tid);
    float best = 0.f, ex = 0.f, ey = 0.f;      // (best from 0 at index 0: a row of zeros matches token 0, the lowest)
    int bj = 0;
    for (int kt = 0; kt < ntiles; ++kt) {
        f32x16 acc[2];
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[jb][r] = 0.f;
        for (int bh = 0; bh < BH; ++bh) {
            const int b = bh / H, h = bh - b * H;
            const size_t boff = (size_t)b * N * ld + h * D;
            QFrags<T, D> qf;
            align_load_q<T, D>(qf, qrow + boff, half);
            const float2 ml = st[(size_t)bh * N];
            __syncthreads();               // the previous step's fragments are read (and, at bh = 0, the previous tile's pos)
            align_k_store<T, D>(lds, sr, kt * KT, N, tid);
            if (bh == 0 && tid < KT) {
                const int j = kt * KT + tid;
                pos[tid] = j < N ? make_float2((float)(j / grid_w), (float)(j % grid_w)) : make_float2(0.f, 0.f);
            }
            __syncthreads();
            {                              // the next step's K rows fly during this step's MFMAs
                const int nbh = bh + 1 < BH ? bh + 1 : 0, nkt = bh + 1 < BH ? kt : kt + 1;
                const int nb = nbh / H, nh = nbh - nb * H;
                if (nkt < ntiles) align_k_load<T, D>(sr, kimg + (size_t)nb * N * ld + nh * D, ld, nkt * KT, N, tid);
            }
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {           // (a block at a time: 16 logits and one block's K fragments live, not 32 and two)
                const f32x16 s = align_logits<T, D>(qf, lds, jb, l31, half);
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[jb][r] = fmaf(__builtin_amdgcn_exp2f(fmaf(s[r], c, ml.x)), ml.y, acc[jb][r]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // the finished tile: mean over (b, h), then best / index / coordinate sums in ascending key order within the lane.  Keys past
        // the end hold 0 and sit at (0, 0): they add nothing and, best starting at 0, never win
        if (kt * KT + KT > N) {
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (kt * KT + align_key(jb, r, half) >= N) acc[jb][r] = 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = align_key(jb, r, half);
                const float v = acc[jb][r] * rbh;
                acc[jb][r] = v;
                const float2 rc = pos[key];
                ex = fmaf(v, rc.x, ex);
                ey = fmaf(v, rc.y, ey);
                if (v > best) { best = v; bj = kt * KT + key; }
            }
        __builtin_amdgcn_sched_barrier(0);
        if (attn && q < N) {
            float* arow = attn + ((size_t)pd * N + q) * N + kt * KT + 4 * half;      // this half's first key of the tile
            const int left = N - kt * KT - 4 * half;                                 // keys from there to the end of the row
            if ((N & 3) == 0) {                  // rows are 16-byte aligned and a group of four lies inside or outside N
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                    for (int r = 0; r < 16; r += 4) {
                        const int off = jb * 32 + 8 * (r >> 2);
                        if (off < left)
                            *reinterpret_cast<f32x4*>(arow + off) = (f32x4){acc[jb][r], acc[jb][r + 1], acc[jb][r + 2], acc[jb][r + 3]};
                    }
            } else {
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int off = jb * 32 + (r & 3) + 8 * (r >> 2);
                        if (off < left) arow[off] = acc[jb][r];
                    }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // the two halves of a row: the larger weight, the lower index on a tie; the coordinate sums lower half first
    const float ob = __shfl_xor(best, 32);
    const int oj = __shfl_xor(bj, 32);
    if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
    ex = half_sum(ex);
    ey = half_sum(ey);
    if (half == 0 && q < N) {
        const size_t o = (size_t)pd * N + q;
        if (match) match[o] = bj;
        if (weight) weight[o] = best;
        if (expect) *reinterpret_cast<float2*>(expect + 2 * o) = make_float2(ex, ey);
        const float t = (ex + ey) + best;                    // a non-finite probability of the row reaches one of the three
        if (status && !(t - t == 0.0f)) status[pair] = 1;
    }
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
