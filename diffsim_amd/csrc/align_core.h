// The two passes of the token alignments as bodies over a row order (attn_core.h's Rows), shared by align.hip (rows in order: the
// whole-image alignments) and region_maps.hip (listed rows: the region alignments); everything here lives in their
// dsim::(anonymous namespace).  They share the tiled core's fragments, MFMA wrappers, K tile geometry and head-dim dispatch
// (attn_core.h), but not attend: there is no V and no O.
//
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
//   align_stats_body    one workgroup per (query tile, b h, pair, direction): the row's final maximum m and denominator
//                       l = sum_j exp2(fma(s, c, -m c)) (online over the key tiles), stored as (-m c, 1 / l): the workspace,
//                       [pair][dir][bh][N] float2, is all that reaches HBM besides the outputs;
//   align_body          one workgroup per (query tile, pair, direction): per 64-key tile, Pm = (sum over (b, h) ascending of
//                       exp2(fma(s, c, -m c)) / l) / (B H), then the finished tile is folded into the lane's running best, its
//                       index and the two coordinate sums (and stored, if attn is asked for).
// A probability depends on its key row only through s, so bit-identical key rows give bit-identical columns of Pm, whichever tile
// or block they fall in.  No atomics: every output element has one writer; status is a plain store of 1 by any row that saw a
// non-finite probability, into a word the launcher zeroed.
//
// Rows.  RowsInOrder: position t of an image is its row t and every image has N of them; list and cnt are not read.  RowsListed:
// the rows of an image i are list[i][0 .. cnt[i]), ascending: query position t is row list[iq][t], key position j row list[ix][j],
// and the images' counts stand where N stood.  Key tiles are formed over positions, so a tile holds the values the in-order body
// holds when run on the compacted tensors, in the same slots: the same MFMA sequence on the same operands, the same probabilities.
// The statistics are stored by position; the outputs go to the query's token list[iq][t], match is the key's token list[ix][j], the
// coordinates are the key token's on the full grid and attn's columns are scattered to the key tokens.  The grid being sized for N, a
// workgroup past the query image's count, or of a pair with an empty image, leaves as a whole before any barrier: its rows are never
// written and never read (the launcher has written the off values).  RowsWeighted (soft_maps.hip): RowsListed, and a key of weight w
// enters both passes with log2(w) added to the exponent, exp2(fma(s, c, -m c) + lb[j]) with m the RAW running maximum; a query token's
// own weight does not enter.  Byte 255 adds + 0.0f: RowsListed's bits.
#pragma once
#include "attn_core.h"

namespace dsim {
namespace {

// this thread's chunks of a K tile on their way from global memory to LDS
template <typename T, int D> struct AlignRegs {
    static constexpr int CPRD = D / ACfg<T, D>::VEC;                 // real 16-B chunks per K row
    static constexpr int N = (KT * CPRD + 255) / 256;
    u32x4 k[N];
};

// (listed rows) the rows of this thread's chunks of one K tile.  They are fetched a tile ahead of the chunks themselves, so that no
// chunk load waits for its index, and serve every (b, h) step of the tile.  Rows in order: empty, never read.
template <typename T, int D, typename Rows> struct AlignRowIdx {
    int32_t row[Rows::LISTED ? AlignRegs<T, D>::N : 1];
    __device__ __forceinline__ void fetch(Rows rows, int kv0, int Nk, int tid) {
        if constexpr (Rows::LISTED) {
            typedef AlignRegs<T, D> SR;
#pragma unroll
            for (int i = 0; i < SR::N; ++i) {
                const int idx = tid + i * 256, r = idx / SR::CPRD;
                if (idx < KT * SR::CPRD && kv0 + r < Nk) row[i] = rows.list[kv0 + r];
            }
        }
    }
};

// the D real columns of key positions kv0 .. kv0 + 63 (those < Nk) of one (image, b, h): global -> registers, registers -> the LDS
// tile (ACfg's K row stride; the padding columns and the never-stored rows keep the zeros of align_zero_tile or stale finite values
// whose logits are masked).  ri (listed rows): the rows of the tile at kv0, from AlignRowIdx::fetch with the same kv0 and Nk
template <typename T, int D, typename Rows>
__device__ __forceinline__ void align_k_load(AlignRegs<T, D>& sr, const T* kb, int ldk, int kv0, int Nk, int tid,
                                             const AlignRowIdx<T, D, Rows>& ri) {
    typedef AlignRegs<T, D> SR;
#pragma unroll
    for (int i = 0; i < SR::N; ++i) {
        const int idx = tid + i * 256, r = idx / SR::CPRD, c = idx - r * SR::CPRD;
        if (idx < KT * SR::CPRD && kv0 + r < Nk) {
            if constexpr (Rows::LISTED)
                sr.k[i] = *reinterpret_cast<const u32x4*>(kb + (size_t)ri.row[i] * ldk + c * ACfg<T, D>::VEC);
            else
                sr.k[i] = *reinterpret_cast<const u32x4*>(kb + (size_t)(kv0 + r) * ldk + c * ACfg<T, D>::VEC);
        }
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

// (weighted rows) the biases of a lane's 16 keys of block jb of key tile kt: slot r = 4 g + e is key position kt*KT + jb*32 + e + 8 g +
// 4 half (align_key), four consecutive positions per 16-byte load; lb is zero padded to whole key tiles, so a ragged tile's loads stay
// inside the row (those logits are -inf already)
__device__ __forceinline__ f32x16 align_key_bias(const float* __restrict__ lb, int kt, int jb, int half) {
    f32x16 b;
    const float* p = lb + kt * KT + jb * 32 + 4 * half;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(p + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) b[4 * g + e] = b4[e];
    }
    return b;
}

// pass 1.  grid (ceil(N/128), B*H, n_pairs*2)
template <typename T, int D, typename Rows>
__device__ __forceinline__ void align_stats_body(const T* __restrict__ qg, const T* __restrict__ kg, const int32_t* __restrict__ list,
                                                 const int32_t* __restrict__ cnt, const int32_t* __restrict__ idx_a,
                                                 const int32_t* __restrict__ idx_b, int B, int H, int N, float c,
                                                 float2* __restrict__ stats, typename Rows::Table wt = typename Rows::Table()) {
    typedef ACfg<T, D> C;
    __shared__ __attribute__((aligned(16))) char lds[C::TILEK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
    const int pair = blockIdx.z >> 1, dir = blockIdx.z & 1;
    const int ia = idx_a[pair], ib = idx_b[pair];
    const int iq = dir ? ib : ia, ix = dir ? ia : ib;
    int nq = N, nk = N;                    // the query image's and the key image's row counts
    Rows rq, rx;
    if constexpr (Rows::LISTED) {
        nq = cnt[iq];
        nk = cnt[ix];
        if ((int)blockIdx.x * 128 >= nq || nk == 0) return;          // (uniform over the workgroup)
        rq.list = list + (size_t)iq * N;
        rx.list = list + (size_t)ix * N;
        if constexpr (Rows::WEIGHTED) rx.lb = wt.lb + (size_t)ix * wt.stride;       // the key image's biases, by key position
    }
    const int ld = H * D;
    const size_t img = (size_t)B * N * ld, boff = (size_t)b * N * ld + h * D;
    const int q = blockIdx.x * 128 + wave * 32 + l31;                // query position
    int qc = q < nq ? q : nq - 1;                                    // its row (a position past the end: the last one's)
    if constexpr (Rows::LISTED) qc = rq.list[qc];
    QFrags<T, D> qf;
    align_load_q<T, D>(qf, qg + iq * img + boff + (size_t)qc * ld, half);
    const T* kb = kg + ix * img + boff;
    const int ntiles = (nk + KT - 1) / KT;
    AlignRegs<T, D> sr;
    AlignRowIdx<T, D, Rows> ri;            // (listed) the rows of the tile whose chunks are loaded next
    ri.fetch(rx, 0, nk, tid);
    align_k_load<T, D>(sr, kb, ld, 0, nk, tid, ri);
    ri.fetch(rx, KT, nk, tid);
    align_zero_tile<T, D>(lds, tid);
    float mc = INFINITY, l = 0.f;          // -m c of the running maximum m (none yet); this half's share of the denominator
    for (int kt = 0; kt < ntiles; ++kt) {
        __syncthreads();                   // the tile is zeroed / the previous tile's fragments are read
        align_k_store<T, D>(lds, sr, kt * KT, nk, tid);
        __syncthreads();
        if (kt + 1 < ntiles) {
            align_k_load<T, D>(sr, kb, ld, (kt + 1) * KT, nk, tid, ri);
            ri.fetch(rx, (kt + 2) * KT, nk, tid);
        }
        f32x16 s[2];
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) s[jb] = align_logits<T, D>(qf, lds, jb, l31, half);
        float tmax = -INFINITY;
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (kt * KT + align_key(jb, r, half) >= nk) s[jb][r] = -INFINITY;
                tmax = fmaxf(tmax, s[jb][r]);
            }
        tmax = max_halves(tmax);
        const float mc_new = fminf(mc, -tmax * c);
        const float alpha = __builtin_amdgcn_exp2f(mc_new - mc);        // tile 0: exp2(-inf) = 0 against l = 0
        mc = mc_new;
        float psum = 0.f;
        if constexpr (Rows::WEIGHTED) {
            // the raw maximum stays the reference point; a key's bias log2(w), in [-7.995, 0], joins the exponent: the maximal key's
            // term is at least 2^-8 and none passes 1
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
                const f32x16 lb = align_key_bias(rx.lb, kt, jb, half);
#pragma unroll
                for (int r = 0; r < 16; ++r) psum += __builtin_amdgcn_exp2f(fmaf(s[jb][r], c, mc) + lb[r]);
            }
        } else {
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int r = 0; r < 16; ++r) psum += __builtin_amdgcn_exp2f(fmaf(s[jb][r], c, mc));
        }
        l = fmaf(l, alpha, psum);
    }
    l = half_sum(l);
    if (half == 0 && q < nq) stats[((size_t)blockIdx.z * gridDim.y + bh) * N + q] = make_float2(mc, 1.0f / l);
}

// pass 2.  grid (ceil(N/128), n_pairs*2)
template <typename T, int D, typename Rows>
__device__ __forceinline__ void align_body(const T* __restrict__ qg, const T* __restrict__ kg, const int32_t* __restrict__ list,
                                           const int32_t* __restrict__ cnt, const int32_t* __restrict__ idx_a,
                                           const int32_t* __restrict__ idx_b, int B, int H, int N, float c, float rbh, int grid_w,
                                           const float2* __restrict__ stats, int32_t* __restrict__ match, float* __restrict__ weight,
                                           float* __restrict__ expect, float* __restrict__ attn, int32_t* __restrict__ status,
                                           typename Rows::Table wt = typename Rows::Table()) {
    typedef ACfg<T, D> C;
    __shared__ __attribute__((aligned(16))) char lds[C::TILEK];
    __shared__ float2 pos[KT];             // (row, col) of the tile's keys on the other image's grid; (0, 0) past the end
    __shared__ int32_t tok[Rows::LISTED ? KT : 1];      // (listed) the tile's key tokens: attn's columns
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int pd = blockIdx.y, pair = pd >> 1, dir = pd & 1;
    const int ia = idx_a[pair], ib = idx_b[pair];
    const int iq = dir ? ib : ia, ix = dir ? ia : ib;
    int nq = N, nk = N;                    // the query image's and the key image's row counts
    Rows rq, rx;
    if constexpr (Rows::LISTED) {
        nq = cnt[iq];
        nk = cnt[ix];
        if ((int)blockIdx.x * 128 >= nq || nk == 0) return;          // (uniform over the workgroup)
        rq.list = list + (size_t)iq * N;
        rx.list = list + (size_t)ix * N;
        if constexpr (Rows::WEIGHTED) rx.lb = wt.lb + (size_t)ix * wt.stride;       // the key image's biases, by key position
    }
    const int BH = B * H, ld = H * D;
    const size_t img = (size_t)B * N * ld;
    const int q = blockIdx.x * 128 + wave * 32 + l31, qp = q < nq ? q : nq - 1;      // query position (past the end: the last one)
    int qc = qp;                                                                      // its row
    if constexpr (Rows::LISTED) qc = rq.list[qp];
    const T* qrow = qg + iq * img + (size_t)qc * ld;
    const T* kimg = kg + ix * img;
    const float2* st = stats + (size_t)pd * BH * N + qp;
    const int ntiles = (nk + KT - 1) / KT;
    AlignRegs<T, D> sr;
    AlignRowIdx<T, D, Rows> ri, rn;        // (listed) the rows of this tile and of the next
    ri.fetch(rx, 0, nk, tid);
    align_k_load<T, D>(sr, kimg, ld, 0, nk, tid, ri);
    align_zero_tile<T, D>(lds, tid);
    float best = 0.f, ex = 0.f, ey = 0.f;      // (best from 0 at index 0: a row of zeros matches position 0, the lowest)
    int bj = 0;
    for (int kt = 0; kt < ntiles; ++kt) {
        f32x16 acc[2];
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[jb][r] = 0.f;
        rn.fetch(rx, (kt + 1) * KT, nk, tid);
        for (int bh = 0; bh < BH; ++bh) {
            const int b = bh / H, h = bh - b * H;
            const size_t boff = (size_t)b * N * ld + h * D;
            QFrags<T, D> qf;
            align_load_q<T, D>(qf, qrow + boff, half);
            const float2 ml = st[(size_t)bh * N];
            __syncthreads();               // the previous step's fragments are read (and, at bh = 0, the previous tile's pos)
            align_k_store<T, D>(lds, sr, kt * KT, nk, tid);
            if (bh == 0 && tid < KT) {
                int j = kt * KT + tid;
                const bool in = j < nk;
                if constexpr (Rows::LISTED) {
                    j = in ? rx.list[j] : 0;
                    tok[tid] = j;
                }
                pos[tid] = in ? make_float2((float)(j / grid_w), (float)(j % grid_w)) : make_float2(0.f, 0.f);
            }
            __syncthreads();
            {                              // the next step's K rows fly during this step's MFMAs
                const int nbh = bh + 1 < BH ? bh + 1 : 0, nkt = bh + 1 < BH ? kt : kt + 1;
                const int nb = nbh / H, nh = nbh - nb * H;
                if (nkt < ntiles) align_k_load<T, D>(sr, kimg + (size_t)nb * N * ld + nh * D, ld, nkt * KT, nk, tid, nkt == kt ? ri : rn);
            }
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {           // (a block at a time: 16 logits and one block's K fragments live, not 32 and two)
                const f32x16 s = align_logits<T, D>(qf, lds, jb, l31, half);
                if constexpr (Rows::WEIGHTED) {
                    const f32x16 lb = align_key_bias(rx.lb, kt, jb, half);
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[jb][r] = fmaf(__builtin_amdgcn_exp2f(fmaf(s[r], c, ml.x) + lb[r]), ml.y, acc[jb][r]);
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[jb][r] = fmaf(__builtin_amdgcn_exp2f(fmaf(s[r], c, ml.x)), ml.y, acc[jb][r]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // the finished tile: mean over (b, h), then best / index / coordinate sums in ascending key order within the lane.  Keys past
        // the end hold 0 and sit at (0, 0): they add nothing and, best starting at 0, never win
        if (kt * KT + KT > nk) {
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (kt * KT + align_key(jb, r, half) >= nk) acc[jb][r] = 0.f;
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
        if (attn && q < nq) {
            if constexpr (Rows::LISTED) {        // the columns are the key tokens: one store per key of the region
                float* arow = attn + ((size_t)pd * N + qc) * N;
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = align_key(jb, r, half);
                        if (kt * KT + key < nk) arow[tok[key]] = acc[jb][r];
                    }
            } else {
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
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (Rows::LISTED) ri = rn;
    }
    // the two halves of a row: the larger weight, the lower index on a tie; the coordinate sums lower half first
    const float ob = __shfl_xor(best, 32);
    const int oj = __shfl_xor(bj, 32);
    if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
    ex = half_sum(ex);
    ey = half_sum(ey);
    if (half == 0 && q < nq) {
        const size_t o = (size_t)pd * N + qc;                // (the query's row: its token)
        if constexpr (Rows::LISTED) bj = rx.list[bj];        // the best key position's token (positions ascend with the tokens)
        if (match) match[o] = bj;
        if (weight) weight[o] = best;
        if (expect) *reinterpret_cast<float2*>(expect + 2 * o) = make_float2(ex, ey);
        const float t = (ex + ey) + best;                    // a non-finite probability of the row reaches one of the three
        if (status && !(t - t == 0.0f)) status[pair] = 1;
    }
}

}  // namespace
}  // namespace dsim
