// Soft score matrices: the region score matrix (region_matrix.hip) with a byte weight per token instead of an on/off bit.  Set A has
// n_a feature images and set B n_b; every image carries weight bytes [N], w = m / 255.  Cell (i, j) is exactly the soft region score
// of the pair (A_i, B_j) as soft_regions.hip defines it (include/diffsim_amd.h, dsim_pair_score_weights), bit for bit: the tokens of
// byte 0 dropped, every softmax with the key image's biases log2(m / 255), a query row's three sums times its byte / 255, the mse
// count from the byte sums.  With bytes 0 / 255 only it is the region matrix's cell on m != 0; with every byte 255 the score matrix's.
//
//   the lists              regions.hip's region_lists_kernel over m != 0, one launch per set into the one list array (set A's images
//                          at index i, set B's at n_a + j), as the region matrix
//   soft_weights_kernel    (soft_core.h) per image: the biases by compacted position and the byte sum; one launch per set likewise
//   cell_index_kernel      (matrix_cells.h) the cells' two images among the n_a + n_b lists, for the finish
//   soft_matrix_kernel     tail_core.h's matrix_tail_kernel with RowsWeighted: the self mode once per image (its own biases, stored at
//                          the compacted position), the cross mode once per cell and direction (the key image's biases; the query
//                          row's weight on the lane's sums)
//   soft_finish_kernel     (soft_core.h) over the cells, through cell_index_kernel's index arrays
// No atomics: every output has one writer, a cell depends on its two images and their weights alone.  The biases stay in global
// memory for soft_regions.hip's reason.  A translation unit of its own for regions.hip's reason: one more attend instantiation per
// head dim and dtype cannot move the register allocation of the kernels that exist.
#include "matrix_cells.h"
#include "soft_core.h"

namespace dsim {
namespace {

// the soft matrix kernel: tail_core.h's matrix_tail_kernel with weighted listed rows (arguments: SoftMatArgs)
// grid  self: (ceil(N/128), B*H, n_a + n_b);  cross: (ceil(N/128) * n_cells * 2, B*H)
template <typename T, int D>
constexpr auto soft_matrix_kernel = matrix_tail_kernel<T, D, RowsWeighted>;

// workspace: MatrixLayout(listed) | biases f32 [n_a + n_b][stride] | byte sums int32 [n_a + n_b], each 256-byte aligned
template <typename T>
int launch_softmat_t(const MatrixArgs& a, float* out, int32_t* status, int32_t* sums, hipStream_t s) {
    const MatrixLayout L(a, sizeof(T), true);
    const int nf = a.n_a + a.n_b;
    char* w = (char*)a.scratch;
    int32_t* list = (int32_t*)w;
    int32_t* cnt = (int32_t*)(w + L.lists);
    int32_t* idx_a = (int32_t*)(w + L.lists + L.counts);
    int32_t* idx_b = (int32_t*)(w + L.lists + L.counts + L.index);
    float* part = (float*)(w + L.parts_at());
    float* lb = (float*)(w + L.total());
    int32_t* sum = (int32_t*)(w + L.total() + soft_bias_bytes(nf, a.N));
    SoftMatArgs m = L.kernel_args<SoftMatArgs>(a);
    m.list = list; m.cnt = cnt; m.lb = lb;
    m.bytes[0] = a.mask[0]; m.bytes[1] = a.mask[1];
    m.stride = soft_stride(a.N);
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        const int qt = (a.N + 127) / 128, nc = a.n_a * a.n_b, BH = a.B * a.H;
        for (int set = 0; set < 2; ++set) {         // the two sets' weights are two arrays: a launch per set, set B's images at n_a + j
            const int n = set ? a.n_b : a.n_a, at = set ? a.n_a : 0;
            const int st = launch_region_lists(a.mask[set], n, a.N, list + (size_t)at * a.N, cnt + at, nullptr, s);
            if (st != DSIM_OK) return st;
            hipLaunchKernelGGL(soft_weights_kernel, dim3(n), dim3(SOFT_THREADS), 0, s, bias_table(), a.mask[set], a.N, m.stride,
                               (const int32_t*)(list + (size_t)at * a.N), (const int32_t*)(cnt + at), lb + (size_t)at * m.stride, sum + at,
                               sums ? sums + at : nullptr);
            DSIM_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(cell_index_kernel, dim3((nc + 255) / 256), dim3(256), 0, s, a.n_a, a.n_b, idx_a, idx_b);
        DSIM_HIP_CHECK(hipGetLastError());
        int st = launch_lds<soft_matrix_kernel<T, Dc>>(dim3(qt, BH, nf), dim3(256), LDS, s, m, scale_log2_of(Dc), a.similarity, 1, part);
        if (st != DSIM_OK) return st;
        st = launch_lds<soft_matrix_kernel<T, Dc>>(dim3(qt * nc * 2, BH), dim3(256), LDS, s, m, scale_log2_of(Dc), a.similarity, 0, part);
        if (st != DSIM_OK) return st;
        hipLaunchKernelGGL(soft_finish_kernel, dim3((nc + 63) / 64), dim3(64), 0, s, (const float*)part, (const int32_t*)sum,
                           (const int32_t*)idx_a, (const int32_t*)idx_b, nc, qt * BH, a.similarity, (double)BH * Dc, out, status);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
// 0 for a call launch_score_matrix_weights refuses for its shape or dtype: the region matrix's refusals, a byte sum that could pass
// int32, and a bias array of 2^31 elements or more
size_t score_matrix_weights_scratch_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    if (!matrix_shape_served(n_a, n_b, B, H, N, D, dtype, true)) return 0;
    if ((long)N * 255 >= (1l << 31) || ((long)n_a + n_b) * soft_stride(N) >= (1l << 31)) return 0;
    return MatrixLayout({{}, {}, {}, {}, n_a, n_b, B, H, N, D}, dtype_size(dtype), true).total() + soft_bias_bytes(n_a + n_b, N) +
           soft_count_bytes(n_a + n_b);
}

// soft score matrix (region_lists_kernel and soft_weights_kernel per set, cell_index_kernel, soft_matrix_kernel twice,
// soft_finish_kernel): any head dim of DSIM_FOR_EACH_D, any N, the three dtypes; a.mask: the two sets' weight bytes
int launch_score_matrix_weights(const MatrixArgs& a, int dtype, float* out, int32_t* status, int32_t* weight_sums, hipStream_t s) {
    const int st = matrix_args_check(a, dtype, true);
    if (st != DSIM_OK) return st;
    const size_t need = score_matrix_weights_scratch_bytes(a.n_a, a.n_b, a.B, a.H, a.N, a.D, dtype);
    if (need == 0) return DSIM_ERR_INVALID;
    if (a.scratch_bytes < need) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype, [&](auto e) { return launch_softmat_t<typename decltype(e)::type>(a, out, status, weight_sums, s); },
        [&] { return DSIM_F16_TWIN(launch_score_matrix_weights(a, dtype, out, status, weight_sums, s)); });
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
