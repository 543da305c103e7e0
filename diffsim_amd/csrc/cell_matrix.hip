// Cell-region score matrices: the region score matrix (region_matrix.hip) and the soft score matrix (soft_matrix.hip) with set B's
// token rows belonging to the CELL, not to the image.  Set A has n_a feature images with a byte row [N] each, set B n_b images, and
// every cell (i, j) brings its own row for B_j: rows_b [n_a][n_b][N].  Cell (i, j) is exactly the region score (bytes: on / off) or
// the soft region score (bytes: weights) of the pair (A_i, B_j) under the rows (rows_a[i], rows_b[i][j]), as regions.hip and
// soft_regions.hip define them, bit for bit.  It is what exemplar-guided retrieval scores: gallery image j has a different region
// against every query i (transfer_matrix.hip makes them).  With rows_b[i][j] equal for all i it is the region / soft matrix's cell.
//
// What a cell can share.  Direction a->b compares SDPA(Q_a[R_a], K_b[R_ij], V_b[R_ij]) with A_i's self attention over R_a, which
// does not depend on the cell: the SELF mode computes it once per set-A image, at compacted positions, and the cell reads it back,
// as the region matrix does.  In direction b->a both attentions run over queries R_ij, so nothing can be kept per image; it runs as
// pair_tail_body's two-attention form -- self, then cross, on one set of Q fragments, the self output rounded and held in registers
// -- and the workspace holds no image-sized slab per cell ("Cell-region score matrices").  A cell costs three attentions.
//
//   the lists              regions.hip's region_lists_kernel (launch_region_lists) over n_a + n_a n_b rows into one list array: set
//                          A's images at index i, the cells' set-B rows at n_a + cell
//   soft_weights_kernel    (soft_core.h; weights only) the biases by compacted position and the byte sums of the same n_a + n_a n_b rows
//   cell_rows_index_kernel idx_a[c] = c / n_b, idx_b[c] = n_a + c: what the finish reads a cell's two counts (byte sums) through
//   cell_matrix_kernel     SELF: set A's self attentions.  CROSS: direction 0 of every cell, matrix_tail_kernel's cross mode with the key
//                          rows of list n_a + cell
//   cell_pair_kernel       direction 1 of every cell: pair_tail_body's text with the query image B_j under list n_a + cell.  Both
//                          kernels run the same attend on the same Q fragments, settle, tail_products and store_block_partial as
//                          the kernels they follow, into their partial layout [cell][dir][bh][qtile][4].  Two kernels and not one
//                          with a branch on the direction: each then allocates registers as the kernel it follows (at head dim 160
//                          cell_pair_kernel has region_tail_kernel's count to the register), and direction 0 does not carry the
//                          two-attention form's
//   the finish             pair_finish_kernel<true> (tail_core.h) or soft_finish_kernel (soft_core.h), unchanged
// No atomics: every output has one writer, a cell depends on its two images and its two rows alone.  The grids are sized for N, the
// counts being on the device.  A translation unit of its own for regions.hip's reason: one more attend instantiation per head dim
// and dtype cannot move the register allocation of the kernels that exist.
#include "soft_core.h"

namespace dsim {
namespace {

// idx_a[c] = c / n_b, idx_b[c] = n_a + c: set A's rows at index i, the cells' set-B rows at n_a + cell
__global__ void cell_rows_index_kernel(int n_a, int n_b, int32_t* __restrict__ idx_a, int32_t* __restrict__ idx_b) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_a * n_b) return;
    idx_a[c] = c / n_b;
    idx_b[c] = n_a + c;
}

// the pointers in front of the extents, as tail_core.h's argument structs and for their reason
struct CellMatArgs {
    const void* q[2]; const void* k[2]; const void* v[2];      // set A, set B: [n][B][N][H*D]
    void* self_a;                                               // set A's self outputs, same layout, rows by compacted position
    const int32_t* list;                                        // [n_a + n_a n_b][N]
    const int32_t* cnt;                                         // [n_a + n_a n_b]
    const float* lb;                                            // (weighted) [n_a + n_a n_b][stride] key biases by compacted position
    const uint8_t* bytes[2];                                    // (weighted) set A's weight bytes [n_a][N], the cells' [n_a n_b][N]
    int n_a, n_b, B, H, N, stride;
};

// SELF: set A's self attentions, one workgroup per (query tile, b h, image).  CROSS: direction 0 of every cell -- A_i's queries over
// B_j's rows of this cell against O_aa read back.  matrix_tail_kernel's text with the key rows of list n_a + cell.
// grid  self: (ceil(N/128), B*H, n_a);  cross: (ceil(N/128) * n_cells, B*H)
// A workgroup whose first position is at or past its query rows' count, or whose key rows are empty, leaves as a whole before any
// barrier (cross: with a zero partial) -- matrix_tail_kernel's rule and order.
template <typename T, int D, typename Rows>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void cell_matrix_kernel(const CellMatArgs p, float scale_log2, int mse, int self_mode,
                                                                                     float* __restrict__ part) {
    static_assert(Rows::LISTED, "the cells' rows come through lists");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
    const int N = p.N, ld = p.H * D;
    const size_t img = (size_t)p.B * N * ld;
    const size_t boff = (size_t)b * N * ld + h * D;
    const int qt = (N + 127) / 128;
    int qtile, iq, ix, cell = 0;                    // iq: the query image in set A; ix: the K / V image (self: iq, cross: in set B)
    int fx;                                         // the K / V rows among the n_a + n_cells lists (the query rows: iq)
    float* o = nullptr;                             // the workgroup's partial (cross)
    if (self_mode) {
        qtile = blockIdx.x;
        fx = iq = ix = blockIdx.z;
    } else {
        cell = blockIdx.x / qt;
        qtile = blockIdx.x - cell * qt;
        iq = cell / p.n_b;
        ix = cell - iq * p.n_b;
        fx = p.n_a + cell;
        o = part + (((size_t)cell * 2 * gridDim.y + bh) * qt + qtile) * 4;
    }
    const int nq = p.cnt[iq], nx = p.cnt[fx];       // the two row counts
    if (qtile * 128 >= nq || nx == 0) {             // (uniform over the workgroup)
        if (!self_mode && threadIdx.x == 0) o[0] = o[1] = o[2] = o[3] = 0.f;
        return;
    }
    Rows rq, rx;
    rq.list = p.list + (size_t)iq * N;
    rx.list = p.list + (size_t)fx * N;
    if constexpr (Rows::WEIGHTED) {
        rq.lb = p.lb + (size_t)iq * p.stride;
        rx.lb = p.lb + (size_t)fx * p.stride;
    }
    const T* qg = (const T*)p.q[0];
    const T* kg = (const T*)p.k[self_mode ? 0 : 1];
    const T* vg = (const T*)p.v[self_mode ? 0 : 1];
    T* so = (T*)p.self_a + iq * img + boff;
    const int t = qtile * 128 + wave * 32 + l31;    // query position
    int q = t < nq ? t : nq - 1;                    // its row (a position past the end: the last one's)
    q = rq.list[q];
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
        const float wq = (float)p.bytes[0][(size_t)iq * N + q] / 255.0f;
        s.s0 *= wq; s.s1 *= wq; s.s2 *= wq;
        asm volatile("" : "+v"(s.s0), "+v"(s.s1), "+v"(s.s2));
    }
    store_block_partial(s, lane, wave, o);
}

// Direction 1 of every cell: B_j's queries over this cell's rows, its self attention and its cross attention over A_i's rows on one
// set of Q fragments, then their products -- pair_tail_body's text (!PER_TOKEN) with the query image B_j under list n_a + cell.
// grid (ceil(N/128) * n_cells, B*H); the early exit as above, pair_tail_body's rule and order.
template <typename T, int D, typename Rows>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void cell_pair_kernel(const CellMatArgs p, float scale_log2, int mse,
                                                                                   float* __restrict__ part) {
    static_assert(Rows::LISTED, "the cells' rows come through lists");
    typedef ACfg<T, D> C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
    const int N = p.N, ld = p.H * D;
    const int qt = (N + 127) / 128;
    const int cell = blockIdx.x / qt, qtile = blockIdx.x - cell * qt;
    const int ix = cell / p.n_b, iq = cell - ix * p.n_b;         // the other image in set A; the query image (also the "self" keys) in set B
    const int fq = p.n_a + cell;                                 // the query rows among the lists (the other image's: ix)
    const int nq = p.cnt[fq], nx = p.cnt[ix];
    float* o = part + ((((size_t)cell * 2 + 1) * gridDim.y + bh) * qt + qtile) * 4;
    if (qtile * 128 >= nq || nx == 0) {                          // (uniform over the workgroup)
        if (threadIdx.x == 0) o[0] = o[1] = o[2] = o[3] = 0.f;
        return;
    }
    Rows rq, rx;
    rq.list = p.list + (size_t)fq * N;
    rx.list = p.list + (size_t)ix * N;
    if constexpr (Rows::WEIGHTED) {
        rq.lb = p.lb + (size_t)fq * p.stride;
        rx.lb = p.lb + (size_t)ix * p.stride;
    }
    const size_t img = (size_t)p.B * N * ld;
    const T* qg = (const T*)p.q[1];
    const T* ks = (const T*)p.k[1];
    const T* vs = (const T*)p.v[1];
    const T* kx = (const T*)p.k[0];
    const T* vx = (const T*)p.v[0];
    const int t = qtile * 128 + wave * 32 + l31;               // query position
    int q = t < nq ? t : nq - 1;                               // its row (a position past the end: the last one's)
    q = rq.list[q];
    const size_t boff = (size_t)b * N * ld + h * D;
    QFrags<T, D> qf;
    load_q<T, D>(qf, qg + iq * img + boff + (size_t)q * ld, half, scale_log2);
    TailSums s;
    if constexpr (sizeof(T) == 2) {
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        h16x2 osp[C::NDB][8];           // the self-attention's output, rounded to the compute dtype, two values per register
        {
            OAcc<T, D> osa;
            attend<T, D, false>(qf, ks + iq * img + boff, vs + iq * img + boff, ld, nq, smem, osa, nullptr, rq, key_bias(rq));
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
        attend<T, D, false>(qf, kx + ix * img + boff, vx + ix * img + boff, ld, nx, smem, oxa, nullptr, rx, key_bias(rx));
        settle<T, D>(oxa);
        if (t < nq) s = tail_products<T, D>(oxa, half, mse, [&](int db, int r, int) { return (float)osp[db][r >> 1][r & 1]; });
    } else {
        OAcc<T, D> osa, oxa;
        attend<T, D, false>(qf, ks + iq * img + boff, vs + iq * img + boff, ld, nq, smem, osa, nullptr, rq, key_bias(rq));
        attend<T, D, false>(qf, kx + ix * img + boff, vx + ix * img + boff, ld, nx, smem, oxa, nullptr, rx, key_bias(rx));
        settle<T, D>(osa);
        settle<T, D>(oxa);
        if (t < nq) s = tail_products<T, D>(oxa, half, mse, [&](int db, int r, int) { return osa.b[db][r]; });
    }
    if constexpr (Rows::WEIGHTED) {
        // the query row's weight on its three sums (byte 255: * 1.0f); pinned, so that the product is rounded on its own
        const float wq = (float)p.bytes[1][(size_t)cell * N + q] / 255.0f;
        s.s0 *= wq; s.s1 *= wq; s.s2 *= wq;
        asm volatile("" : "+v"(s.s0), "+v"(s.s1), "+v"(s.s2));
    }
    store_block_partial(s, lane, wave, o);
}

// workspace, each part 256-byte aligned:
//   lists int32 [n_a + n_cells][N] | counts int32 [n_a + n_cells] | cell indices int32 [2][n_cells] | self A |
//   partials f32 [n_cells][2][B H][qtiles][4] | (weights) biases f32 [n_a + n_cells][stride] | byte sums int32 [n_a + n_cells]
struct CellLayout {
    size_t lists, counts, index, self_a, parts, bias = 0, sums = 0;
    CellLayout(int n_a, int n_b, int B, int H, int N, int D, size_t es, bool weighted) {
        const size_t nc = (size_t)n_a * n_b, nr = n_a + nc;
        lists = up256(nr * N * sizeof(int32_t));
        counts = up256(nr * sizeof(int32_t));
        index = up256(nc * sizeof(int32_t));
        self_a = up256((size_t)n_a * B * N * H * D * es);
        parts = up256(nc * 2 * B * H * ((N + 127) / 128) * 4 * sizeof(float));
        if (weighted) {
            bias = up256(nr * soft_stride(N) * sizeof(float));
            sums = up256(nr * sizeof(int32_t));
        }
    }
    size_t self_at() const { return lists + counts + 2 * index; }
    size_t parts_at() const { return self_at() + self_a; }
    size_t bias_at() const { return parts_at() + parts; }
    size_t total() const { return bias_at() + bias + sums; }
};

// the cell matrices' own refusals, on the host: the region matrix's with n_a + n_a n_b rows where it has n_a + n_b
bool cell_shape_served(int n_a, int n_b, int B, int H, int N, int D, int dtype, bool weighted) {
    if (dtype != DSIM_F32 && dtype != DSIM_BF16 && dtype != DSIM_F16) return false;
    if (n_a < 1 || n_b < 1 || B < 1 || H < 1 || N < 1) return false;
    if (with_head_dim(D, [](auto) { return DSIM_OK; }) != DSIM_OK) return false;
    const long lim = 1l << 31, qt = (N + 127) / 128, nc = (long)n_a * n_b, bh = (long)B * H;
    if ((long)n_a + n_b > 65535 || bh > 65535 || nc * 2 * qt >= lim) return false;
    const long row = bh * D, mx = n_a > n_b ? n_a : n_b;                      // (row < 2^16 * 2^8)
    if (row >= lim / N || row * N >= lim / mx) return false;                  // a set's q, k, v and set A's self output
    if ((n_a + nc) * N >= lim) return false;                                  // the lists, and the cells' rows
    if (nc * 2 * qt >= lim / (bh * 4)) return false;                          // the partials
    if (weighted && ((long)N * 255 >= lim || (n_a + nc) * soft_stride(N) >= lim)) return false;      // a byte sum, the biases
    return true;
}

template <typename T, typename Rows>
int launch_cells_t(const MatrixArgs& a, float* out, int32_t* status, int32_t* extra, hipStream_t s) {
    const CellLayout L(a.n_a, a.n_b, a.B, a.H, a.N, a.D, sizeof(T), Rows::WEIGHTED);
    const int nc = a.n_a * a.n_b;
    char* w = (char*)a.scratch;
    int32_t* list = (int32_t*)w;
    int32_t* cnt = (int32_t*)(w + L.lists);
    int32_t* idx_a = (int32_t*)(w + L.lists + L.counts);
    int32_t* idx_b = (int32_t*)(w + L.lists + L.counts + L.index);
    float* part = (float*)(w + L.parts_at());
    float* lb = (float*)(w + L.bias_at());
    int32_t* sum = (int32_t*)(w + L.bias_at() + L.bias);
    CellMatArgs m{};
    for (int set = 0; set < 2; ++set) { m.q[set] = a.q[set]; m.k[set] = a.k[set]; m.v[set] = a.v[set]; m.bytes[set] = a.mask[set]; }
    m.self_a = w + L.self_at();
    m.list = list; m.cnt = cnt; m.lb = lb;
    m.n_a = a.n_a; m.n_b = a.n_b; m.B = a.B; m.H = a.H; m.N = a.N; m.stride = soft_stride(a.N);
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        const int qt = (a.N + 127) / 128, BH = a.B * a.H;
        for (int set = 0; set < 2; ++set) {         // set A's rows and the cells' are two arrays: a launch each, the cells' at n_a + cell
            const int n = set ? nc : a.n_a, at = set ? a.n_a : 0;
            const int st = launch_region_lists(a.mask[set], n, a.N, list + (size_t)at * a.N, cnt + at,
                                               !Rows::WEIGHTED && extra ? extra + at : nullptr, s);
            if (st != DSIM_OK) return st;
            if constexpr (Rows::WEIGHTED) {
                hipLaunchKernelGGL(soft_weights_kernel, dim3(n), dim3(SOFT_THREADS), 0, s, bias_table(), a.mask[set], a.N, m.stride,
                                   (const int32_t*)(list + (size_t)at * a.N), (const int32_t*)(cnt + at), lb + (size_t)at * m.stride, sum + at,
                                   extra ? extra + at : nullptr);
                DSIM_HIP_CHECK(hipGetLastError());
            }
        }
        hipLaunchKernelGGL(cell_rows_index_kernel, dim3((nc + 255) / 256), dim3(256), 0, s, a.n_a, a.n_b, idx_a, idx_b);
        DSIM_HIP_CHECK(hipGetLastError());
        int st = launch_lds<cell_matrix_kernel<T, Dc, Rows>>(dim3(qt, BH, a.n_a), dim3(256), LDS, s, m, scale_log2_of(Dc), a.similarity, 1, part);
        if (st != DSIM_OK) return st;
        st = launch_lds<cell_matrix_kernel<T, Dc, Rows>>(dim3(qt * nc, BH), dim3(256), LDS, s, m, scale_log2_of(Dc), a.similarity, 0, part);
        if (st != DSIM_OK) return st;
        st = launch_lds<cell_pair_kernel<T, Dc, Rows>>(dim3(qt * nc, BH), dim3(256), LDS, s, m, scale_log2_of(Dc), a.similarity, part);
        if (st != DSIM_OK) return st;
        if constexpr (Rows::WEIGHTED) {
            hipLaunchKernelGGL(soft_finish_kernel, dim3((nc + 63) / 64), dim3(64), 0, s, (const float*)part, (const int32_t*)sum,
                               (const int32_t*)idx_a, (const int32_t*)idx_b, nc, qt * BH, a.similarity, (double)BH * Dc, out, status);
            DSIM_HIP_CHECK(hipGetLastError());
            return DSIM_OK;
        } else {
            return launch_pair_finish<true>(part, cnt, idx_a, idx_b, nc, qt * BH, a.similarity, (double)BH * Dc, out, status, s);
        }
    });
}

int launch_cells(const MatrixArgs& a, int dtype, bool weighted, float* out, int32_t* status, int32_t* extra, hipStream_t s) {
    if (a.similarity != 0 && a.similarity != 1) return DSIM_ERR_INVALID;
    if (!cell_shape_served(a.n_a, a.n_b, a.B, a.H, a.N, a.D, dtype, weighted)) return DSIM_ERR_INVALID;
    if (a.scratch_bytes < CellLayout(a.n_a, a.n_b, a.B, a.H, a.N, a.D, dtype_size(dtype), weighted).total()) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype,
        [&](auto e) {
            typedef typename decltype(e)::type T;
            return weighted ? launch_cells_t<T, RowsWeighted>(a, out, status, extra, s) : launch_cells_t<T, RowsListed>(a, out, status, extra, s);
        },
        [&] {
            return weighted ? DSIM_F16_TWIN(launch_score_matrix_cell_weights(a, dtype, out, status, extra, s))
                            : DSIM_F16_TWIN(launch_score_matrix_cell_regions(a, dtype, out, status, extra, s));
        });
}

}  // namespace

inline namespace DSIM_H16_NS {
// 0 for a call the launchers refuse for its shape or dtype
size_t score_matrix_cell_regions_scratch_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    if (!cell_shape_served(n_a, n_b, B, H, N, D, dtype, false)) return 0;
    return CellLayout(n_a, n_b, B, H, N, D, dtype_size(dtype), false).total();
}
size_t score_matrix_cell_weights_scratch_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    if (!cell_shape_served(n_a, n_b, B, H, N, D, dtype, true)) return 0;
    return CellLayout(n_a, n_b, B, H, N, D, dtype_size(dtype), true).total();
}

// cell-region score matrix (region_lists_kernel twice, cell_rows_index_kernel, cell_matrix_kernel twice, cell_pair_kernel, pair_finish_kernel<true>):
// any head dim of DSIM_FOR_EACH_D, any N, the three dtypes; a.mask[0]: set A's masks [n_a][N], a.mask[1]: the cells' [n_a][n_b][N]
int launch_score_matrix_cell_regions(const MatrixArgs& a, int dtype, float* out, int32_t* status, int32_t* counts, hipStream_t s) {
    return launch_cells(a, dtype, false, out, status, counts, s);
}
// ... and with weight bytes (soft_weights_kernel per row array, soft_finish_kernel): the soft matrix's arithmetic
int launch_score_matrix_cell_weights(const MatrixArgs& a, int dtype, float* out, int32_t* status, int32_t* weight_sums, hipStream_t s) {
    return launch_cells(a, dtype, true, out, status, weight_sums, s);
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
