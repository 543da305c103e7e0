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
//   cell_index_kernel      (matrix_cells.h) idx_a[c] = c / n_b, idx_b[c] = n_a + c % n_b: what the finish reads the two counts of a cell through
//   region_matrix_kernel   the score matrix's kernel (tails.hip launches it with the rows in order) -- the same source text,
//                          tail_core.h's matrix_tail_kernel: the self mode once per image, the cross mode once per cell and
//                          direction -- instantiated with the rows taken through the lists (RowsListed): the images' counts where
//                          N stood, the self outputs at compacted positions
//   the finish             pair_finish_kernel<true> (tail_core.h), unchanged
// No atomics: every output has one writer, a cell depends on its two images alone.  The grids are sized for N, the counts being on
// the device (the worst case, as region_tail_kernel's).  A translation unit of its own for regions.hip's reason: one more attend
// instantiation per head dim and dtype cannot move the register allocation of the kernels that exist.
#include "matrix_cells.h"

namespace dsim {
namespace {

// the region matrix kernel: tail_core.h's matrix_tail_kernel with listed rows (arguments: RegMatArgs)
// grid  self: (ceil(N/128), B*H, n_a + n_b);  cross: (ceil(N/128) * n_cells * 2, B*H)
template <typename T, int D>
constexpr auto region_matrix_kernel = matrix_tail_kernel<T, D, RowsListed>;

template <typename T>
int launch_regmat_t(const MatrixArgs& a, float* out, int32_t* status, int32_t* counts, hipStream_t s) {
    const MatrixLayout L(a, sizeof(T), true);
    char* w = (char*)a.scratch;
    int32_t* list = (int32_t*)w;
    int32_t* cnt = (int32_t*)(w + L.lists);
    int32_t* idx_a = (int32_t*)(w + L.lists + L.counts);
    int32_t* idx_b = (int32_t*)(w + L.lists + L.counts + L.index);
    float* part = (float*)(w + L.parts_at());
    RegMatArgs m = L.kernel_args<RegMatArgs>(a);
    m.list = list; m.cnt = cnt;
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        const int qt = (a.N + 127) / 128, nc = a.n_a * a.n_b, BH = a.B * a.H;
        // the two sets' masks are two arrays: a launch per set into the one list array, set B's images at index n_a + j
        int st = launch_region_lists(a.mask[0], a.n_a, a.N, list, cnt, counts, s);
        if (st != DSIM_OK) return st;
        st = launch_region_lists(a.mask[1], a.n_b, a.N, list + (size_t)a.n_a * a.N, cnt + a.n_a, counts ? counts + a.n_a : nullptr, s);
        if (st != DSIM_OK) return st;
        hipLaunchKernelGGL(cell_index_kernel, dim3((nc + 255) / 256), dim3(256), 0, s, a.n_a, a.n_b, idx_a, idx_b);
        DSIM_HIP_CHECK(hipGetLastError());
        st = launch_lds<region_matrix_kernel<T, Dc>>(dim3(qt, BH, a.n_a + a.n_b), dim3(256), LDS, s, m, scale_log2_of(Dc), a.similarity, 1, part);
        if (st != DSIM_OK) return st;
        st = launch_lds<region_matrix_kernel<T, Dc>>(dim3(qt * nc * 2, BH), dim3(256), LDS, s, m, scale_log2_of(Dc), a.similarity, 0, part);
        if (st != DSIM_OK) return st;
        return launch_pair_finish<true>(part, cnt, idx_a, idx_b, nc, qt * BH, a.similarity, (double)BH * Dc, out, status, s);
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
// 0 for a call launch_score_matrix_regions refuses for its shape or dtype
size_t score_matrix_regions_scratch_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    if (!matrix_shape_served(n_a, n_b, B, H, N, D, dtype, true)) return 0;
    return MatrixLayout({{}, {}, {}, {}, n_a, n_b, B, H, N, D}, dtype_size(dtype), true).total();
}

// region score matrix (region_lists_kernel, cell_index_kernel, region_matrix_kernel twice, pair_finish_kernel<true>): any head dim
// of DSIM_FOR_EACH_D, any N, the three dtypes; the default tap runs the tiled kernel too
int launch_score_matrix_regions(const MatrixArgs& a, int dtype, float* out, int32_t* status, int32_t* counts, hipStream_t s) {
    const int st = matrix_args_check(a, dtype, true);
    if (st != DSIM_OK) return st;
    if (a.scratch_bytes < score_matrix_regions_scratch_bytes(a.n_a, a.n_b, a.B, a.H, a.N, a.D, dtype)) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype, [&](auto e) { return launch_regmat_t<typename decltype(e)::type>(a, out, status, counts, s); },
        [&] { return DSIM_F16_TWIN(launch_score_matrix_regions(a, dtype, out, status, counts, s)); });
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
