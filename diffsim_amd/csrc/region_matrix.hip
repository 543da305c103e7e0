// Region score matrices: every image of set A against every image of set B, each image restricted to a token region.  Set A has n_a
// feature images and set B n_b; every image carries a byte mask [N] (non-zero = on) with region R_i.  Cell (i, j) is exactly the
// region score of the pair (A_i, B_j) as regions.hip defines it: rows in ascending token order, both SDPAs over the regions' rows
// only, outputs rounded to the pipeline dtype, cosine with F.cosine_similarity's eps or mse divided by B H |R_query| D, the mean of
// the two directions.  With all masks full it is the score matrix's cell (tails.hip); a cell with an empty region on either side is
// NaN with status 2 and disturbs no other cell; rows outside a region are never read.
//
//   the lists              regions.hip's region_lists_kernel (through launch_region_lists, the one source of it) over the n_a + n_b
//                          masks into one list array: set A's images at index i, set B's at n_a + j.  The two sets' masks arrive as
//                          two arrays, so it is one launch per set
//   cell_index_kernel      idx_a[c] = c / n_b, idx_b[c] = n_a + c % n_b: what the finish reads the two counts of a cell through
//   region_matrix_kernel   matrix_tail_kernel's two modes (tails.hip) over listed rows.  SELF: attend of an image over its own listed
//                          rows, stored at the COMPACTED position t (row t of the image's slab holds token list[t]), so that CROSS
//                          reads it back by position without an index load.  CROSS: one attention per cell and direction, query rows
//                          through the query image's list, K / V rows through the partner's, the counts where N stood; the pair
//                          tail's products and partial layout [cell][dir][bh][qtile][4]
//   the finish             pair_finish_kernel<true> (tail_core.h), unchanged
// No atomics: every output has one writer, a cell depends on its two images alone.  The grids are sized for N, the counts being on
// the device (the worst case, as region_tail_kernel's).  A translation unit of its own for regions.hip's reason: one more attend
// instantiation per head dim and dtype cannot move the register allocation of the kernels that exist.
#include "tail_core.h"

namespace dsim {
namespace {

struct RegMatArgs {
    const void* q[2]; const void* k[2]; const void* v[2];      // set A, set B: [n][B][N][H*D]
    void* self[2];                                              // the sets' self outputs, same layout, rows by compacted position
    const int32_t* list;                                        // [n_a + n_b][N]
    const int32_t* cnt;                                         // [n_a + n_b]
    int n_a, n_b, B, H, N;
};

// grid  self: (ceil(N/128), B*H, n_a + n_b);  cross: (ceil(N/128) * n_cells * 2, B*H)
// A SELF workgroup whose first position is at or past its image's count leaves as a whole before any barrier: its rows are never
// written and never read.  A CROSS workgroup past the query image's count, or of a cell with an empty image, writes a zero partial
// and leaves -- pair_tail_body's rule and order: uniform over the workgroup, before any barrier, thread 0 stores.
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void region_matrix_kernel(const RegMatArgs p, float scale_log2, int mse, int self_mode,
                                                                                       float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
    const int N = p.N, ld = p.H * D;
    const size_t img = (size_t)p.B * N * ld;
    const size_t boff = (size_t)b * N * ld + h * D;
    const int qt = (N + 127) / 128;
    int qtile, set, iq, ix, fq, fx;          // iq, ix: the images inside their sets; fq, fx: among the n_a + n_b lists
    float* o = nullptr;                      // the workgroup's partial (cross)
    if (self_mode) {
        qtile = blockIdx.x;
        fq = fx = blockIdx.z;
        set = fq >= p.n_a;
        iq = ix = fq - (set ? p.n_a : 0);
    } else {
        qtile = blockIdx.x % qt;
        const int cd = blockIdx.x / qt;
        const int cell = cd >> 1, dir = cd & 1;
        const int ia = cell / p.n_b, ib = cell - ia * p.n_b;
        set = dir;
        iq = dir ? ib : ia;
        ix = dir ? ia : ib;
        fq = dir ? p.n_a + ib : ia;
        fx = dir ? ia : p.n_a + ib;
        o = part + ((((size_t)cell * 2 + dir) * gridDim.y + bh) * qt + qtile) * 4;
    }
    const int nq = p.cnt[fq], nx = p.cnt[fx];                  // the two images' row counts
    if (qtile * 128 >= nq || nx == 0) {                        // (uniform over the workgroup)
        if (!self_mode && threadIdx.x == 0) o[0] = o[1] = o[2] = o[3] = 0.f;
        return;
    }
    RowsListed rq, rx;
    rq.list = p.list + (size_t)fq * N;
    rx.list = p.list + (size_t)fx * N;
    const T* qg = (const T*)p.q[set];
    const T* kg = (const T*)p.k[set ^ (self_mode ? 0 : 1)];
    const T* vg = (const T*)p.v[set ^ (self_mode ? 0 : 1)];
    T* so = (T*)p.self[set] + iq * img + boff;
    const int t = qtile * 128 + wave * 32 + l31;               // query position
    const int q = rq.list[t < nq ? t : nq - 1];                // its row (a position past the end: the last one's)
    QFrags<T, D> qf;
    load_q<T, D>(qf, qg + iq * img + boff + (size_t)q * ld, half, scale_log2);
    OAcc<T, D> oa;
    attend<T, D, false, RowsListed>(qf, kg + ix * img + boff, vg + ix * img + boff, ld, nx, smem, oa, nullptr, rx);
    settle<T, D>(oa);
    if (self_mode) {
        if (t < nq) fold_rounded<T, D>(oa, half, 0, [&](int, int, int, int d, T y) { so[(size_t)t * ld + d] = y; return 0; });  // (no state)
        return;
    }
    TailSums s;
    if (t < nq) s = tail_products<T, D>(oa, half, mse, [&](int, int, int d) { return (float)so[(size_t)t * ld + d]; });
    store_block_partial(s, lane, wave, o);
}

// the cells' images among the n_a + n_b lists, for pair_finish_kernel<true>
__global__ void cell_index_kernel(int n_a, int n_b, int32_t* __restrict__ idx_a, int32_t* __restrict__ idx_b) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_a * n_b) return;
    idx_a[c] = c / n_b;
    idx_b[c] = n_a + c % n_b;
}

// workspace: [lists int32 [n_a + n_b][N] | counts int32 [n_a + n_b] | cell indices int32 [2][n_cells] | self A | self B |
// partials f32 [n_cells][2][B H][qtiles][4]], each 256-byte aligned
struct RegMatLayout {
    size_t lists, counts, index, self_a, self_b, parts;
    size_t total() const { return lists + counts + 2 * index + self_a + self_b + parts; }
};
RegMatLayout regmat_layout(int n_a, int n_b, int B, int H, int N, int D, size_t es) {
    const size_t nf = (size_t)n_a + n_b, nc = (size_t)n_a * n_b, row = (size_t)B * N * H * D * es;
    return {up256(nf * N * sizeof(int32_t)), up256(nf * sizeof(int32_t)), up256(nc * sizeof(int32_t)), up256(n_a * row), up256(n_b * row),
            up256(nc * 2 * B * H * ((N + 127) / 128) * 4 * sizeof(float))};
}

// The calls served: a dtype of the three, a head dim of DSIM_FOR_EACH_D, at least one image per set, one token, one head; n_a + n_b
// and B*H each on a 65535-wide grid axis; the cross grid in a 32-bit extent; every tensor and list under 2^31 elements
bool regmat_served(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    if (dtype != DSIM_F32 && dtype != DSIM_BF16 && dtype != DSIM_F16) return false;
    if (n_a < 1 || n_b < 1 || B < 1 || H < 1 || N < 1 || D < 1) return false;
    if (with_head_dim(D, [](auto) { return DSIM_OK; }) != DSIM_OK) return false;
    if ((long)n_a + n_b > 65535 || (long)B * H > 65535) return false;
    const long lim = 1l << 31, qt = (N + 127) / 128, nc = (long)n_a * n_b, mx = n_a > n_b ? n_a : n_b;
    if (nc >= lim / (2 * qt)) return false;                                      // the cross grid
    const long row = (long)B * H * D;                                            // (< 2^16 * 2^8)
    if (row >= lim / N || row * N >= lim / mx) return false;                     // a set's q, k, v and self output
    if (((long)n_a + n_b) * N >= lim) return false;                              // the lists
    if (nc * 2 * qt >= lim / ((long)B * H * 4)) return false;                    // the partials
    return true;
}

template <typename T>
int launch_regmat_t(const void* qa, const void* ka, const void* va, const uint8_t* mask_a, int n_a, const void* qb, const void* kb,
                    const void* vb, const uint8_t* mask_b, int n_b, int B, int H, int N, int D, int mse, float* out, int32_t* status,
                    int32_t* counts, void* scratch, hipStream_t s) {
    const RegMatLayout L = regmat_layout(n_a, n_b, B, H, N, D, sizeof(T));
    char* w = (char*)scratch;
    int32_t* list = (int32_t*)w;          w += L.lists;
    int32_t* cnt = (int32_t*)w;           w += L.counts;
    int32_t* idx_a = (int32_t*)w;         w += L.index;
    int32_t* idx_b = (int32_t*)w;         w += L.index;
    RegMatArgs m;
    m.q[0] = qa; m.k[0] = ka; m.v[0] = va; m.q[1] = qb; m.k[1] = kb; m.v[1] = vb;
    m.self[0] = w;                        w += L.self_a;
    m.self[1] = w;                        w += L.self_b;
    float* part = (float*)w;
    m.list = list; m.cnt = cnt;
    m.n_a = n_a; m.n_b = n_b; m.B = B; m.H = H; m.N = N;
    return with_head_dim(D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        const int qt = (N + 127) / 128, nc = n_a * n_b;
        // the two sets' masks are two arrays: a launch per set into the one list array, set B's images at index n_a + j
        int st = launch_region_lists(mask_a, n_a, N, list, cnt, counts, s);
        if (st != DSIM_OK) return st;
        st = launch_region_lists(mask_b, n_b, N, list + (size_t)n_a * N, cnt + n_a, counts ? counts + n_a : nullptr, s);
        if (st != DSIM_OK) return st;
        hipLaunchKernelGGL(cell_index_kernel, dim3((nc + 255) / 256), dim3(256), 0, s, n_a, n_b, idx_a, idx_b);
        DSIM_HIP_CHECK(hipGetLastError());
        st = launch_lds<region_matrix_kernel<T, Dc>>(dim3(qt, B * H, n_a + n_b), dim3(256), LDS, s, m, scale_log2_of(Dc), mse, 1, part);
        if (st != DSIM_OK) return st;
        st = launch_lds<region_matrix_kernel<T, Dc>>(dim3(qt * nc * 2, B * H), dim3(256), LDS, s, m, scale_log2_of(Dc), mse, 0, part);
        if (st != DSIM_OK) return st;
        hipLaunchKernelGGL(pair_finish_kernel<true>, dim3((nc + 63) / 64), dim3(64), 0, s, (const float*)part, (const int32_t*)cnt,
                           (const int32_t*)idx_a, (const int32_t*)idx_b, nc, qt * B * H, mse, (double)B * H * Dc, out, status);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
// 0 for a call launch_score_matrix_regions refuses for its shape or dtype
size_t score_matrix_regions_scratch_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    if (!regmat_served(n_a, n_b, B, H, N, D, dtype)) return 0;
    return regmat_layout(n_a, n_b, B, H, N, D, dtype == DSIM_F32 ? 4 : 2).total();
}

// region score matrix (region_lists_kernel, cell_index_kernel, region_matrix_kernel twice, pair_finish_kernel<true>): any head dim
// of DSIM_FOR_EACH_D, any N, the three dtypes; the default tap runs the tiled kernel too
int launch_score_matrix_regions(const void* qa, const void* ka, const void* va, const uint8_t* mask_a, int n_a, const void* qb,
                                const void* kb, const void* vb, const uint8_t* mask_b, int n_b, int B, int H, int N, int D, int dtype,
                                int similarity, float* out, int32_t* status, int32_t* counts, void* scratch, size_t scratch_bytes,
                                hipStream_t s) {
    if (similarity != 0 && similarity != 1) return DSIM_ERR_INVALID;
    const size_t need = score_matrix_regions_scratch_bytes(n_a, n_b, B, H, N, D, dtype);
    if (need == 0) return DSIM_ERR_INVALID;
    if (scratch_bytes < need) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype,
        [&](auto e) {
            return launch_regmat_t<typename decltype(e)::type>(qa, ka, va, mask_a, n_a, qb, kb, vb, mask_b, n_b, B, H, N, D, similarity, out,
                                                               status, counts, scratch, s);
        },
        [&] {
            return DSIM_F16_TWIN(launch_score_matrix_regions(qa, ka, va, mask_a, n_a, qb, kb, vb, mask_b, n_b, B, H, N, D, dtype, similarity,
                                                             out, status, counts, scratch, scratch_bytes, s));
        });
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
