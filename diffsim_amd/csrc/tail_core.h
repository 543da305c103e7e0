// What the score tails share on top of the tiled attention core (attn_core.h): the rounding of attend's output to the pipeline
// dtype, the products of a cross output against a self output, a workgroup's partial, the two-attention pair body (pair_tail_body:
// tails.hip's pair and map kernels in row order, regions.hip's region tail and region_maps.hip's region map kernel through row
// lists), the one-attention matrix kernel
// (matrix_tail_kernel: tails.hip's score matrix in row order, region_matrix.hip's through row lists, soft_matrix.hip's through
// weighted row lists) with its arguments and
// workspace layout, and the f64 finishes (direction_value, store_score, pair_finish_kernel, pair_map_finish_kernel and their
// launches).  Shared by tails.hip (pairs, maps, matrices), regions.hip (region scores), region_matrix.hip (region matrices) and
// region_maps.hip (region maps), which must round and multiply alike
// to agree bit for bit; everything here lives in their dsim::(anonymous namespace).
#pragma once
#include "attn_core.h"

namespace dsim {
namespace {

// ---- fused score tail ----------------------------------------------------------------------
// 16-bit modes (round 5): both SDPA outputs are rounded to the compute dtype before the products -- torch's SDPA returns
// tensors of the pipeline dtype and the reference's cosine / mse consume those (diffsim.py:177-190); the products and sums stay
// f32 per workgroup and f64 across them.  The self-attention's output then waits for the cross-attention as packed 16-bit
// pairs (40 registers at d = 160 instead of 80), which brings d = 160 from 426 registers (one workgroup per CU) under 256: two
// workgroups per CU.  The f32 parity mode keeps both outputs in f32.

// attend's output in the lane's row, rounded to the compute dtype T (the 16-bit modes convert two values at a time), folded in
// slot order: s = f(s, db, r, d, x) for every accumulator slot (db, r) whose column d is < D.  (The state goes through f by value:
// with the current compiler, sums held by reference across the walk move the register allocation of the tail kernels.)
template <typename T, int D, typename S, typename F>
__device__ __forceinline__ S fold_rounded(const OAcc<T, D>& acc, int half, S s, F&& f) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int db = 0; db < ACfg<T, D>::NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            T v[2];
            if constexpr (sizeof(T) == 2) {
                const h16x2 p = __builtin_convertvector((f32x2){acc.b[db][r], acc.b[db][r + 1]}, h16x2);
                v[0] = p[0]; v[1] = p[1];
            } else {
                v[0] = acc.b[db][r]; v[1] = acc.b[db][r + 1];
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int rr = r + e, d = db * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * half;
                if (d < D) s = f(s, db, rr, d, v[e]);
            }
        }
    return s;
}

// attend's normalised output held as plain f32 values: hipcc may otherwise fuse attend's final multiply by 1/l into what consumes
// it -- into the fp16 rounding (v_fma_mixlo_f16: one rounding instead of f32 then fp16) or into the mse difference (an fma) -- and it
// does so in some tail kernels and not in others.  Every tail calls it on every attend output, so that pair_tail_body and
// matrix_tail_kernel round and subtract the same f32 values and a matrix cell equals the pair tail's score bit for bit.
template <typename T, int D>
__device__ __forceinline__ void settle(OAcc<T, D>& acc) {
#pragma unroll
    for (int db = 0; db < ACfg<T, D>::NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (db * 32 + (r & 3) + 8 * (r >> 2) >= D) continue;      // (no lane holds a column d < D in this slot)
            float x = acc.b[db][r];
            asm volatile("" : "+v"(x));
            acc.b[db][r] = x;
        }
}

// the products of the cross output ox (rounded by fold_rounded) against the self output y(db, r, d), in f32: cosine sums
// dot | x2 | y2 into s0 | s1 | s2, mse the squared difference into s0
struct TailSums { float s0 = 0.f, s1 = 0.f, s2 = 0.f; };
template <typename T, int D, typename Y>
__device__ __forceinline__ TailSums tail_products(const OAcc<T, D>& ox, int half, int mse, Y&& y) {
    return fold_rounded<T, D>(ox, half, TailSums{}, [&](TailSums s, int db, int r, int d, T xr) {
        const float x = (float)xr, yv = y(db, r, d);
        if (mse) { const float df = x - yv; s.s0 = fmaf(df, df, s.s0); }
        else { s.s0 = fmaf(x, yv, s.s0); s.s1 = fmaf(x, x, s.s1); s.s2 = fmaf(yv, yv, s.s2); }
        return s;
    });
}

// a workgroup's products folded over its 4 waves (shuffles, then the waves in a fixed order) into its partial
// o[0..3] = (s0, s1, s2, 0); every thread of the workgroup calls it
__device__ __forceinline__ void store_block_partial(TailSums t, int lane, int wave, float* __restrict__ o) {
    __shared__ float red[4][4];
    float s0 = t.s0, s1 = t.s1, s2 = t.s2;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_xor(s0, off);
        s1 += __shfl_xor(s1, off);
        s2 += __shfl_xor(s2, off);
    }
    if (lane == 0) { red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        o[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
        o[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
        o[2] = (red[0][2] + red[1][2]) + (red[2][2] + red[3][2]);
        o[3] = 0.f;
    }
}

// One direction of a pair in a 128-query workgroup: the self and the cross attention on the same Q fragments, then their products.
// The epilogue is one partial per workgroup, [pair][dir][bh][qtile][4] f32 (PER_TOKEN false), or one per query token,
// [pair][dir][comp][bh][N] f32 indexed by query POSITION, comp: dot | x2 | y2, or sqd | - | - (PER_TOKEN true).
// Rows (attn_core.h): RowsInOrder -- query position t of an image is its row t and every image has N of them; list and cnt are not
// read.  RowsListed -- the rows of an image i are list[i][0 .. cnt[i]), ascending: position t is row list[i][t] and the image's count
// stands where N stood; the grid being sized for N, a workgroup past the query image's count, or of a pair with an empty image,
// writes a zero partial and leaves as a whole before any barrier (PER_TOKEN: it writes nothing -- the positions from the count on
// are never written, and the finish never reads them).  RowsWeighted (soft_regions.hip) -- RowsListed, and both attends add the key
// image's log2 weights to the logits (key_bias) and a query row's three sums are multiplied by its weight byte / 255 (wt: the
// call's weights); with every listed byte 255 the additions are + 0.0f and the factor is 1.0f: RowsListed's bits.
// grid (ceil(N/128), B*H, n_pairs*2)
template <typename T, int D, bool PER_TOKEN, typename Rows>
__device__ __forceinline__ void pair_tail_body(const T* __restrict__ qg, const T* __restrict__ kg, const T* __restrict__ vg,
                                               const int32_t* __restrict__ list, const int32_t* __restrict__ cnt,
                                               const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_b, int B, int H, int N,
                                               float scale_log2, int mse, float* __restrict__ part,
                                               typename Rows::Table wt = typename Rows::Table()) {
    typedef ACfg<T, D> C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
    const int pair = blockIdx.z >> 1, dir = blockIdx.z & 1;
    const int ia = idx_a[pair], ib = idx_b[pair];
    const int iq = dir ? ib : ia;        // query image (also the "self" keys/values)
    const int ix = dir ? ia : ib;        // the other image ("cross" keys/values)
    int nq = N, nx = N;                  // the two images' row counts
    Rows rq, rx;
    float* o = nullptr;                  // the workgroup's partial
    if constexpr (Rows::LISTED) {
        nq = cnt[iq];
        nx = cnt[ix];
        if constexpr (!PER_TOKEN) o = part + ((((size_t)pair * 2 + dir) * gridDim.y + bh) * gridDim.x + blockIdx.x) * 4;
        if ((int)blockIdx.x * 128 >= nq || nx == 0) {          // (uniform over the workgroup)
            if constexpr (!PER_TOKEN)
                if (threadIdx.x == 0) o[0] = o[1] = o[2] = o[3] = 0.f;
            return;
        }
        rq.list = list + (size_t)iq * N;
        rx.list = list + (size_t)ix * N;
        if constexpr (Rows::WEIGHTED) {
            rq.lb = wt.lb + (size_t)iq * wt.stride;
            rx.lb = wt.lb + (size_t)ix * wt.stride;
        }
    }
    const int ld = H * D;
    const size_t img = (size_t)B * N * ld;
    const int t = blockIdx.x * 128 + wave * 32 + l31;          // query position
    int q = t < nq ? t : nq - 1;                               // its row (a position past the end: the last one's)
    if constexpr (Rows::LISTED) q = rq.list[q];
    const size_t boff = (size_t)b * N * ld + h * D;
    QFrags<T, D> qf;
    load_q<T, D>(qf, qg + iq * img + boff + (size_t)q * ld, half, scale_log2);
    TailSums s;
    if constexpr (sizeof(T) == 2) {
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        h16x2 osp[C::NDB][8];           // the self-attention's output, rounded to the compute dtype, two values per register
        {
            OAcc<T, D> osa;
            attend<T, D, false>(qf, kg + iq * img + boff, vg + iq * img + boff, ld, nq, smem, osa, nullptr, rq, key_bias(rq));
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
        attend<T, D, false>(qf, kg + ix * img + boff, vg + ix * img + boff, ld, nx, smem, oxa, nullptr, rx, key_bias(rx));
        settle<T, D>(oxa);
        if (t < nq) s = tail_products<T, D>(oxa, half, mse, [&](int db, int r, int) { return (float)osp[db][r >> 1][r & 1]; });
    } else {
        OAcc<T, D> osa, oxa;
        attend<T, D, false>(qf, kg + iq * img + boff, vg + iq * img + boff, ld, nq, smem, osa, nullptr, rq, key_bias(rq));
        attend<T, D, false>(qf, kg + ix * img + boff, vg + ix * img + boff, ld, nx, smem, oxa, nullptr, rx, key_bias(rx));
        settle<T, D>(osa);
        settle<T, D>(oxa);
        if (t < nq) s = tail_products<T, D>(oxa, half, mse, [&](int db, int r, int) { return osa.b[db][r]; });
    }
    if constexpr (Rows::WEIGHTED && !PER_TOKEN) {
        // the query row's weight on its three sums (byte 255: * 1.0f); pinned, so that the product is rounded on its own and never
        // fused into the additions that follow.  (Per token the partials stay unweighted: pair_map_finish_kernel applies the weight.)
        const float wq = (float)wt.bytes[(size_t)iq * N + q] / 255.0f;
        s.s0 *= wq; s.s1 *= wq; s.s2 *= wq;
        asm volatile("" : "+v"(s.s0), "+v"(s.s1), "+v"(s.s2));
    }
    if constexpr (PER_TOKEN) {
        // a row's d values are split between the two lane halves: fold them, then the first half stores the row at its position
        // t < nq (rows in order: nq = N) -- 128 B per wave and component, no atomics
        const float s0 = s.s0 + __shfl_xor(s.s0, 32);
        const float s1 = s.s1 + __shfl_xor(s.s1, 32);
        const float s2 = s.s2 + __shfl_xor(s.s2, 32);
        if (half == 0 && t < nq) {
            const size_t plane = (size_t)gridDim.y * N;
            float* po = part + ((size_t)pair * 2 + dir) * 3 * plane + (size_t)bh * N + t;
            po[0] = s0;
            if (!mse) { po[plane] = s1; po[2 * plane] = s2; }
        }
    } else {
        if constexpr (!Rows::LISTED) o = part + ((((size_t)pair * 2 + dir) * gridDim.y + bh) * gridDim.x + blockIdx.x) * 4;
        store_block_partial(s, lane, wave, o);
    }
}

// ---- score matrices ------------------------------------------------------------------------------------------------------------
// Every image of set A against every image of set B.  The score of (a, b) needs O_aa and O_bb, which do not depend on the partner:
// they are computed once per image and read back by every cell.  The kernel arguments with the rows in order, and with listed rows:
// the same fields and the lists and counts (the in-order kernel carries no pointer it never reads).  A struct of its own, the two
// pointers in front of the extents: with them behind, as a derived struct puts them, hipcc groups the listed kernel's scalar argument
// loads otherwise, and that form measured 1.3 % slower at (N, H, D) = (1024, 8, 80) (profiles/matrix_tail_refactor.json,
// "earlier_forms").
struct MatArgs {
    const void* q[2]; const void* k[2]; const void* v[2];      // set A, set B: [n][B][N][H*D]
    void* self[2];                                              // the sets' self outputs, same layout (listed: rows by compacted position)
    int n_a, n_b, B, H, N;
};
struct RegMatArgs {
    const void* q[2]; const void* k[2]; const void* v[2];
    void* self[2];
    const int32_t* list;                                        // [n_a + n_b][N]: set A's images at index i, set B's at n_a + j
    const int32_t* cnt;                                         // [n_a + n_b]
    int n_a, n_b, B, H, N;
};
// ... and with weighted rows (soft_matrix.hip): RegMatArgs, the key biases by compacted position, the sets' weight bytes and the
// biases' row stride; the pointers in front of the extents likewise
struct SoftMatArgs {
    const void* q[2]; const void* k[2]; const void* v[2];
    void* self[2];
    const int32_t* list;
    const int32_t* cnt;
    const float* lb;                                            // [n_a + n_b][stride]: log2(byte / 255) of the listed tokens, zero padded
    const uint8_t* bytes[2];                                    // set A, set B: [n][N] weight bytes on the token grid
    int n_a, n_b, B, H, N, stride;
};

// One attention of a 128-query workgroup, in one of two modes.  SELF: an image's self attention (rounded to the compute dtype as the
// pair tail rounds it; f32 in the parity mode) into [n][B][N][H*D].  CROSS: one attention per cell and direction -- O_ab = SDPA(Qa, Kb,
// Vb) against O_aa read back, O_ba = SDPA(Qb, Ka, Va) against O_bb -- with the pair tail's products, reduction and partial layout
// [cell][dir][bh][qtile][4], so pair_finish_kernel folds them.  Both modes run the same attend on the same Q fragments as
// pair_tail_body: a cell of an image against itself compares bit-identical tensors, and a cell equals the pair tail's score of the
// same two images.
// Rows as pair_tail_body's.  RowsInOrder: tails.hip's score matrix (matrix_tail_kernel<T, D, RowsInOrder>).  RowsListed:
// region_matrix.hip's region matrix (its region_matrix_kernel<T, D> names that instantiation): the counts stand where N stood; SELF
// stores at the COMPACTED position t (row t of the image's slab holds token list[t]), so that CROSS reads it back by position without
// an index load; a SELF workgroup whose first position is at or past its image's count leaves as a whole before any barrier (its rows
// are never written and never read), a CROSS workgroup past the query image's count, or of a cell with an empty image, writes a zero
// partial and leaves likewise -- pair_tail_body's rule and order.  RowsWeighted: soft_matrix.hip's soft matrix (arguments:
// SoftMatArgs): RowsListed, every attend with the key image's biases (SELF: the image's own), and CROSS multiplies the lane's three
// sums by the query row's byte / 255, pinned as pair_tail_body pins it; every byte 255: RowsListed's bits.
// The shared text is the kernel itself, not an inline body under two wrapper kernels: hipcc optimises such a body as a function of
// its own before it inlines it, and the kernels then come out in another instruction order than written directly ("Region
// score matrices").  Each translation unit instantiates only the row order it launches.  Args is a parameter only so that the symbol
// names the argument struct: it is MatrixKernelArgs<Rows>, nothing else.
// grid  self: (ceil(N/128), B*H, n_a + n_b);  cross: (ceil(N/128) * n_cells * 2, B*H)
template <typename Rows>
using MatrixKernelArgs = std::conditional_t<Rows::WEIGHTED, SoftMatArgs, std::conditional_t<Rows::LISTED, RegMatArgs, MatArgs>>;
template <typename T, int D, typename Rows, typename Args = MatrixKernelArgs<Rows>>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void matrix_tail_kernel(const Args p, float scale_log2, int mse, int self_mode,
                                                                                     float* __restrict__ part) {
    static_assert(std::is_same<Args, MatrixKernelArgs<Rows>>::value, "the in-order kernel takes MatArgs, the listed one RegMatArgs, the weighted one SoftMatArgs");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
    const int N = p.N, ld = p.H * D;
    const size_t img = (size_t)p.B * N * ld;
    const size_t boff = (size_t)b * N * ld + h * D;
    const int qt = (N + 127) / 128;
    int qtile, set, iq, ix, cell = 0, dir = 0;      // iq, ix: the query image and the K / V image inside their sets
    int fq = 0, fx = 0;                             // (listed) the same two among the n_a + n_b lists
    float* o = nullptr;                             // the workgroup's partial (cross)
    if (self_mode) {
        qtile = blockIdx.x;
        fq = fx = blockIdx.z;
        set = fq >= p.n_a;
        iq = ix = fq - (set ? p.n_a : 0);
    } else {
        qtile = blockIdx.x % qt;
        const int cd = blockIdx.x / qt;
        cell = cd >> 1; dir = cd & 1;
        const int ia = cell / p.n_b, ib = cell - ia * p.n_b;
        set = dir;
        iq = dir ? ib : ia;
        ix = dir ? ia : ib;
        if constexpr (Rows::LISTED) {
            fq = dir ? p.n_a + ib : ia;
            fx = dir ? ia : p.n_a + ib;
            o = part + ((((size_t)cell * 2 + dir) * gridDim.y + bh) * qt + qtile) * 4;
        }
    }
    int nq = N, nx = N;                             // the two images' row counts
    Rows rq, rx;
    if constexpr (Rows::LISTED) {
        nq = p.cnt[fq];
        nx = p.cnt[fx];
        if (qtile * 128 >= nq || nx == 0) {         // (uniform over the workgroup)
            if (!self_mode && threadIdx.x == 0) o[0] = o[1] = o[2] = o[3] = 0.f;
            return;
        }
        rq.list = p.list + (size_t)fq * N;
        rx.list = p.list + (size_t)fx * N;
        if constexpr (Rows::WEIGHTED) {
            rq.lb = p.lb + (size_t)fq * p.stride;
            rx.lb = p.lb + (size_t)fx * p.stride;
        }
    }
    const T* qg = (const T*)p.q[set];
    const T* kg = (const T*)p.k[set ^ (self_mode ? 0 : 1)];
    const T* vg = (const T*)p.v[set ^ (self_mode ? 0 : 1)];
    T* so = (T*)p.self[set] + iq * img + boff;
    const int t = qtile * 128 + wave * 32 + l31;    // query position
    int q = t < nq ? t : nq - 1;                    // its row (a position past the end: the last one's)
    if constexpr (Rows::LISTED) q = rq.list[q];
    QFrags<T, D> qf;
    load_q<T, D>(qf, qg + iq * img + boff + (size_t)q * ld, half, scale_log2);
    OAcc<T, D> oa;
    attend<T, D, false>(qf, kg + ix * img + boff, vg + ix * img + boff, ld, nx, smem, oa, nullptr, rx, key_bias(rx));
    settle<T, D>(oa);
    if (self_mode) {
        if (t < nq) fold_rounded<T, D>(oa, half, 0, [&](int, int, int, int d, T y) { so[(size_t)t * ld + d] = y; return 0; });  // (no state)
        return;
    }
    TailSums s;
    if (t < nq) s = tail_products<T, D>(oa, half, mse, [&](int, int, int d) { return (float)so[(size_t)t * ld + d]; });
    if constexpr (Rows::WEIGHTED) {
        // the query row's weight on its three sums, rounded on its own (pair_tail_body's lines; a lane past the count holds zero
        // sums and the last listed row's byte: the product is zero, as there)
        const float wq = (float)p.bytes[set][(size_t)iq * N + q] / 255.0f;
        s.s0 *= wq; s.s1 *= wq; s.s2 *= wq;
        asm volatile("" : "+v"(s.s0), "+v"(s.s1), "+v"(s.s2));
    }
    if constexpr (!Rows::LISTED) o = part + ((((size_t)cell * 2 + dir) * gridDim.y + bh) * qt + qtile) * 4;
    store_block_partial(s, lane, wave, o);
}

// workspace of a tiled score matrix, each part 256-byte aligned:
//   [lists int32 [n_a + n_b][N] | counts int32 [n_a + n_b] | cell indices int32 [2][n_cells] |]   (listed only)
//   self A | self B | partials f32 [n_cells][2][B H][qtiles][4]
struct MatrixLayout {
    size_t lists = 0, counts = 0, index = 0, self_a, self_b, parts;
    MatrixLayout(const MatrixArgs& a, size_t es, bool listed) {
        const size_t nf = (size_t)a.n_a + a.n_b, nc = (size_t)a.n_a * a.n_b, image = (size_t)a.B * a.N * a.H * a.D * es;
        if (listed) {
            lists = up256(nf * a.N * sizeof(int32_t));
            counts = up256(nf * sizeof(int32_t));
            index = up256(nc * sizeof(int32_t));
        }
        self_a = up256(a.n_a * image);
        self_b = up256(a.n_b * image);
        parts = up256(nc * 2 * a.B * a.H * ((a.N + 127) / 128) * 4 * sizeof(float));
    }
    size_t self_at() const { return lists + counts + 2 * index; }
    size_t parts_at() const { return self_at() + self_a + self_b; }
    size_t total() const { return parts_at() + parts; }
    // the kernels' arguments (MatArgs, or RegMatArgs less its list and cnt) over a's workspace
    template <typename Args>
    Args kernel_args(const MatrixArgs& a) const {
        Args m{};
        for (int set = 0; set < 2; ++set) { m.q[set] = a.q[set]; m.k[set] = a.k[set]; m.v[set] = a.v[set]; }
        m.self[0] = (char*)a.scratch + self_at();
        m.self[1] = (char*)m.self[0] + self_a;
        m.n_a = a.n_a; m.n_b = a.n_b; m.B = a.B; m.H = a.H; m.N = a.N;
        return m;
    }
};

// ---- the f64 finish ------------------------------------------------------------------------------------------------------------
// A direction's value from the f64 folds of its partials (diffsim.py:187-197): mse a / count, cosine a / (|x| |y|) with
// F.cosine_similarity's eps = 1e-8 under each norm.  The denominator alone for a caller that divides many numerators by it.
__device__ __forceinline__ double direction_denominator(double x2, double y2, int mse, double count) {
    if (mse) return count;
    return fmax(sqrt(x2), 1e-8) * fmax(sqrt(y2), 1e-8);
}
__device__ __forceinline__ double direction_value(double a, double x2, double y2, int mse, double count) {
    return a / direction_denominator(x2, y2, mse, count);
}
// the score, the mean of the two directions' values, and its status (NaN guard: non-finite features surface here as a non-finite
// score; 1 reports it)
__device__ __forceinline__ void store_score(double both, float* __restrict__ out, int32_t* __restrict__ status) {
    const float sc = (float)(both * 0.5);
    *out = sc;
    if (status) *status = (sc - sc == 0.0f) ? 0 : 1;
}

// One thread per pair: fixed-order f64 fold of the workgroups' partials [pair][dir][nblk][4], then the two directions' values and
// their mean.  REGIONS false: count = a direction's elements B H N D.  REGIONS true (regions.hip; the partials of the workgroups that
// left are zeros): count = B H D, the elements per row, times the query image's own row count; a pair with an empty image: NaN and
// status 2.  cnt, idx_a and idx_b are read only then.
template <bool REGIONS>
__global__ void pair_finish_kernel(const float* __restrict__ part, const int32_t* __restrict__ cnt, const int32_t* __restrict__ idx_a,
                                   const int32_t* __restrict__ idx_b, int n_pairs, int nblk, int mse, double count,
                                   float* __restrict__ out, int32_t* __restrict__ status) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    int n[2] = {1, 1};
    if constexpr (REGIONS) {
        n[0] = cnt[idx_a[p]];
        n[1] = cnt[idx_b[p]];
        if (n[0] == 0 || n[1] == 0) {
            out[p] = __builtin_nanf("");
            if (status) status[p] = 2;
            return;
        }
    }
    double res = 0.0;
    for (int dir = 0; dir < 2; ++dir) {
        double a = 0.0, x2 = 0.0, y2 = 0.0;
        const float* o = part + ((size_t)p * 2 + dir) * nblk * 4;
        for (int i = 0; i < nblk; ++i) { a += o[4 * i]; x2 += o[4 * i + 1]; y2 += o[4 * i + 2]; }
        res += direction_value(a, x2, y2, mse, REGIONS ? count * n[dir] : count);
    }
    store_score(res, out + p, status ? status + p : nullptr);
}

// pair_finish_kernel over n items (pairs or cells) of nblk partials per direction: its one launch site
template <bool REGIONS>
int launch_pair_finish(const float* part, const int32_t* cnt, const int32_t* idx_a, const int32_t* idx_b, int n, int nblk, int mse,
                       double count, float* out, int32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(pair_finish_kernel<REGIONS>, dim3((n + 63) / 64), dim3(64), 0, s, part, cnt, idx_a, idx_b, n, nblk, mse, count, out,
                       status);
    DSIM_HIP_CHECK(hipGetLastError());
    return DSIM_OK;
}

// ---- the f64 finish of the per-token partials ------------------------------------------------------------------------------------
// one workgroup per pair, both directions: per token, a fixed-order f64 fold of the B*H partials; over tokens, per-thread strided
// sums and a fixed-order tree.  local: the token's own cosine (|.| of the token's vectors) or mean squared difference; contrib: its
// share of the direction's score, so that 0.5 (sum contrib[0] + sum contrib[1]) is the pair's score (the finish arithmetic above,
// as pair_finish_kernel).
// Rows as pair_tail_body's.  RowsInOrder (tails.hip's similarity maps): the partials' N positions are the tokens; mask, list, cnt,
// idx_a and idx_b are not read.  RowsListed (region_maps.hip's region maps): the folds run over the positions t < cnt of the
// direction's query image -- the same strided sums and tree, so that full masks give the in-order bits -- each result goes to token
// list[t], and the thread that owns an off token (mask byte 0) stores its zeros: every element of local and contrib has one writer.
// The mse count of a direction is B H D times the query image's own count, as pair_finish_kernel<true>'s.  A pair with an empty
// image: score NaN, status 2, both maps zero.  RowsWeighted (soft_maps.hip's soft maps): RowsListed with mask holding the weight
// bytes; the partials arrive unweighted, local is the token's own value, and both folds apply the query token's byte / 255 in f64:
// the squared norms and contrib carry it, the mse count is B H D (byte sum) / 255; bytes 0 / 255: factors of exactly 1, the listed bits.
constexpr int MAP_FINISH_THREADS = 256;
template <typename Rows>
__global__ __launch_bounds__(MAP_FINISH_THREADS) void pair_map_finish_kernel(const float* __restrict__ part, const uint8_t* __restrict__ mask,
                                                                             const int32_t* __restrict__ list, const int32_t* __restrict__ cnt,
                                                                             const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_b,
                                                                             int BH, int N, int D, int mse, float* __restrict__ score,
                                                                             float* __restrict__ local, float* __restrict__ contrib,
                                                                             int32_t* __restrict__ status) {
    constexpr int NT = MAP_FINISH_THREADS;
    __shared__ double red[3][NT];
    const int p = blockIdx.x, t = threadIdx.x;
    const size_t plane = (size_t)BH * N;
    int img[2] = {0, 0}, n[2] = {N, N};        // (listed) the directions' query images and their counts
    if constexpr (Rows::LISTED) {
        img[0] = idx_a[p]; img[1] = idx_b[p];
        n[0] = cnt[img[0]]; n[1] = cnt[img[1]];
        if (n[0] == 0 || n[1] == 0) {          // (uniform over the workgroup)
            for (int i = t; i < 2 * N; i += NT) {
                if (local) local[(size_t)p * 2 * N + i] = 0.f;
                if (contrib) contrib[(size_t)p * 2 * N + i] = 0.f;
            }
            if (t == 0) {
                score[p] = __builtin_nanf("");
                if (status) status[p] = 2;
            }
            return;
        }
    }
    double res = 0.0;
    for (int dir = 0; dir < 2; ++dir) {
        const float* pd = part + ((size_t)p * 2 + dir) * 3 * plane;
        float* lo = local ? local + ((size_t)p * 2 + dir) * N : nullptr;
        float* co = contrib ? contrib + ((size_t)p * 2 + dir) * N : nullptr;
        const int nd = n[dir];
        const int32_t* lst = nullptr;
        const uint8_t* wb = nullptr;             // (weighted) the query image's weight bytes
        double wsum = 0.0;                       // (weighted) their sum / 255
        if constexpr (Rows::LISTED) {
            lst = list + (size_t)img[dir] * N;
            const uint8_t* m = mask + (size_t)img[dir] * N;
            for (int i = t; i < N; i += NT)
                if (m[i] == 0) {
                    if (lo) lo[i] = 0.f;
                    if (co) co[i] = 0.f;
                }
            if constexpr (Rows::WEIGHTED) {
                wb = m;
                double bs = 0.0;                 // the byte sum: integers in f64, exact in any order
                for (int i = t; i < N; i += NT) bs += (double)m[i];
                red[0][t] = bs;
                __syncthreads();
                for (int s = NT / 2; s > 0; s >>= 1) {
                    if (t < s) red[0][t] += red[0][t + s];
                    __syncthreads();
                }
                wsum = red[0][0] / 255.0;
                __syncthreads();
            }
        }
        auto token = [&](int i) {                // the token of position i
            if constexpr (Rows::LISTED) return (int)lst[i];
            else return i;
        };
        auto fold = [&](int comp, int i) {
            double a = 0.0;
            for (int j = 0; j < BH; ++j) a += pd[comp * plane + (size_t)j * N + i];
            return a;
        };
        auto wof = [&](int i) {                  // (weighted) the weight of position i, byte / 255 in f64 (byte 255: exactly 1)
            if constexpr (Rows::WEIGHTED) return (double)wb[lst[i]] / 255.0;
            else return 1.0;
        };
        // pass 1: local, and the direction's squared norms (cosine)
        double x2t = 0.0, y2t = 0.0;
        for (int i = t; i < nd; i += NT) {
            const double a = fold(0, i);
            if (mse) {                   // (mse folds no norms)
                if (lo) lo[token(i)] = (float)direction_value(a, 0.0, 0.0, mse, (double)BH * D);
            } else {
                const double x2 = fold(1, i), y2 = fold(2, i);
                if constexpr (Rows::WEIGHTED) { const double w = wof(i); x2t += w * x2; y2t += w * y2; }
                else { x2t += x2; y2t += y2; }
                if (lo) lo[token(i)] = (float)direction_value(a, x2, y2, mse, (double)BH * D);
            }
        }
        red[1][t] = x2t; red[2][t] = y2t;
        __syncthreads();
        for (int s = NT / 2; s > 0; s >>= 1) {
            if (t < s) { red[1][t] += red[1][t + s]; red[2][t] += red[2][t + s]; }
            __syncthreads();
        }
        double den;
        if constexpr (Rows::WEIGHTED) den = direction_denominator(red[1][0], red[2][0], mse, (double)BH * D * wsum);
        else den = direction_denominator(red[1][0], red[2][0], mse, (double)BH * nd * D);
        // pass 2: contrib (the same fold again: the per-token sums are not kept), and the direction's total
        double ct = 0.0;
        for (int i = t; i < nd; i += NT) {
            double c;
            if constexpr (Rows::WEIGHTED) c = wof(i) * fold(0, i) / den;
            else c = fold(0, i) / den;
            ct += c;
            if (co) co[token(i)] = (float)c;
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

// pair_map_finish_kernel over a's pairs at head dim D: its one launch site
template <typename Rows>
int launch_map_finish(const float* part, const uint8_t* mask, const int32_t* list, const int32_t* cnt, const PairArgs& a, int D,
                      float* score, float* local, float* contrib, int32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(pair_map_finish_kernel<Rows>, dim3(a.n_pairs), dim3(MAP_FINISH_THREADS), 0, s, part, mask, list, cnt, a.idx_a, a.idx_b,
                       a.B * a.H, a.N, D, a.similarity, score, local, contrib, status);
    DSIM_HIP_CHECK(hipGetLastError());
    return DSIM_OK;
}

}  // namespace
}  // namespace dsim
