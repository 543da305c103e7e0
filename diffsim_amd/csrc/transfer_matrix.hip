// Transfer matrix: the attention mass every image of set B sends into every set-A image's weighted tokens.  Set A has n_a feature
// images with weight bytes [n_a][N], set B n_b images without any.  Cell (i, j) is the region transfer's mirror row of the pair
// (a = A_i, b = B_j) as transfer.hip defines it, bit for bit:
//   mass[i][j][u] = sum_t Pm_ba[u][t] w_a[t]      (B_j's queries over A_i's keys, weighted by A_i's bytes / 255)
// with Pm the token alignments' attention (align_core.h).  It is what exemplar-guided retrieval needs of the transfer: every gallery
// image's region against every query's mask, in one launch, the two sets in tensors of their own.
//
//   transfer_cell_kernel   transfer.hip's transfer_part_kernel with the images addressed by cell instead of through pair indices and
//                          one direction only: one workgroup per (query tile of 128, cell, b h).  The arithmetic text is that
//                          kernel's, line by line -- align_logits on the same operands, the online maximum, l and num with the same
//                          fma order, r_bh = num / l -- so that a cell equals the pair form's row.  A kernel of its own and not a body
//                          shared with transfer_part_kernel: hipcc optimises such a body as a function of its own before it inlines
//                          it ("Region score matrices"), and the pair kernel must keep the code it has.
//                          part[cell][bh][N] f32 is the whole workspace: the pair form's second direction does not exist here.
//   transfer_cell_fold_kernel   one thread per output element: mass = (sum over bh ascending of r_bh) * (1 / (B H)), status[cell] = 1
//                          (a plain store into a word the launcher zeroed) where that is not finite.
// No atomics, one writer per element; a cell's row depends on its two images and A_i's weights alone.  The cells ride on the grid's
// x axis beside the query tiles, so n_a * n_b is not bound by a grid extent of 65535.
#include "align_core.h"

namespace dsim {
namespace {

// grid (ceil(N/128) * n_a * n_b, B*H)
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void transfer_cell_kernel(const T* __restrict__ qb, const T* __restrict__ ka,
                                                               const uint8_t* __restrict__ wa, int n_b, int B, int H, int N, float c,
                                                               float* __restrict__ part) {
    typedef ACfg<T, D> C;
    __shared__ __attribute__((aligned(16))) char lds[C::TILEK];
    __shared__ __attribute__((aligned(16))) float wl[KT];        // the tile's key weights; 0 past the end
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
    const int qt = (N + 127) / 128;
    const int cell = blockIdx.x / qt, qtile = blockIdx.x - cell * qt;
    const int ix = cell / n_b, iq = cell - ix * n_b;                 // the key image in set A, the query image in set B
    const int ld = H * D;
    const size_t img = (size_t)B * N * ld, boff = (size_t)b * N * ld + h * D;
    const int q = qtile * 128 + wave * 32 + l31;                     // query position (past the end: the last one's row)
    const int qc = q < N ? q : N - 1;
    QFrags<T, D> qf;
    align_load_q<T, D>(qf, qb + iq * img + boff + (size_t)qc * ld, half);
    const T* kb = ka + ix * img + boff;
    const uint8_t* wb = wa + (size_t)ix * N;
    const int ntiles = (N + KT - 1) / KT;
    AlignRegs<T, D> sr;
    const AlignRowIdx<T, D, RowsInOrder> ri = {};
    align_k_load<T, D, RowsInOrder>(sr, kb, ld, 0, N, tid, ri);
    float wn = 0.f;                        // (tid < KT) this thread's key weight of the tile staged next
    if (tid < KT && tid < N) wn = (float)wb[tid] / 255.0f;
    align_zero_tile<T, D>(lds, tid);
    float mc = INFINITY, l = 0.f, num = 0.f;      // -m c of the running maximum m (none yet); this half's shares of the two sums
    for (int kt = 0; kt < ntiles; ++kt) {
        __syncthreads();                   // the tile is zeroed / the previous tile's fragments and weights are read
        align_k_store<T, D>(lds, sr, kt * KT, N, tid);
        if (tid < KT) wl[tid] = wn;
        __syncthreads();
        if (kt + 1 < ntiles) {
            align_k_load<T, D, RowsInOrder>(sr, kb, ld, (kt + 1) * KT, N, tid, ri);
            const int j = (kt + 1) * KT + tid;
            if (tid < KT) wn = j < N ? (float)wb[j] / 255.0f : 0.f;
        }
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
        const float alpha = __builtin_amdgcn_exp2f(mc_new - mc);        // tile 0: exp2(-inf) = 0 against sums of 0
        mc = mc_new;
        float psum = 0.f, nsum = 0.f;
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {      // slot r = 4 g + e is key jb*32 + e + 8 g + 4 half (align_key): four consecutive weights
                const f32x4 w4 = *reinterpret_cast<const f32x4*>(wl + jb * 32 + 8 * g + 4 * half);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(s[jb][4 * g + e], c, mc));
                    psum += p;
                    nsum = fmaf(p, w4[e], nsum);
                }
            }
        l = fmaf(l, alpha, psum);
        num = fmaf(num, alpha, nsum);
    }
    l = half_sum(l);
    num = half_sum(num);
    if (half == 0 && q < N) part[((size_t)cell * gridDim.y + bh) * N + q] = num / l;
}

// one thread per (cell, token)
__global__ __launch_bounds__(256) void transfer_cell_fold_kernel(const float* __restrict__ part, int n_cells, int BH, int N, float rbh,
                                                                 float* __restrict__ mass, int32_t* __restrict__ status) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n_cells * N) return;
    const int i = (int)(t % N);
    const size_t cell = t / N;
    const float* p = part + cell * BH * N + i;
    float total = 0.f;
    for (int bh = 0; bh < BH; ++bh) total += p[(size_t)bh * N];
    const float v = total * rbh;
    mass[cell * N + i] = v;
    // (the exponent bits, as transfer_fold_kernel tests them and for its reason)
    if (status && (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) status[cell] = 1;
}

template <typename T>
int launch_transfer_matrix_t(const MatrixArgs& a, float* mass, int32_t* status, hipStream_t s) {
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value;
        const int qt = (a.N + 127) / 128, nc = a.n_a * a.n_b, BH = a.B * a.H;
        if (status) DSIM_HIP_CHECK(hipMemsetAsync(status, 0, (size_t)nc * sizeof(int32_t), s));
        hipLaunchKernelGGL((transfer_cell_kernel<T, Dc>), dim3(qt * nc, BH), dim3(256), 0, s, (const T*)a.q[1], (const T*)a.k[0], a.mask[0],
                           a.n_b, a.B, a.H, a.N, scale_log2_of(Dc), (float*)a.scratch);
        DSIM_HIP_CHECK(hipGetLastError());
        const size_t total = (size_t)nc * a.N;
        hipLaunchKernelGGL(transfer_cell_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)a.scratch, nc, BH,
                           a.N, 1.0f / (float)BH, mass, status);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
// the partials of transfer_cell_kernel, [cell][bh][N] f32; 0 for a call the launcher does not serve: a dtype outside the three, an
// extent below 1, a head dim outside DSIM_FOR_EACH_D, n_a + n_b > 65535, a grid extent (B H on y, the query tiles times the cells on
// x), or a tensor of 2^31 elements or more (a set's features, the weights, the masses, the partials)
size_t region_transfer_matrix_scratch_bytes(int n_a, int n_b, int B, int H, int N, int D, int dtype) {
    if (dtype != DSIM_F32 && dtype != DSIM_BF16 && dtype != DSIM_F16) return 0;
    if (n_a < 1 || n_b < 1 || B < 1 || H < 1 || N < 1) return 0;
    if (with_head_dim(D, [](auto) { return DSIM_OK; }) != DSIM_OK) return 0;
    const long lim = 1l << 31, qt = (N + 127) / 128, nc = (long)n_a * n_b, bh = (long)B * H;
    if ((long)n_a + n_b > 65535 || bh > 65535) return 0;
    const long row = bh * D, mx = n_a > n_b ? n_a : n_b;                  // (row < 2^16 * 2^8)
    if (row >= lim / N || row * N >= lim / mx) return 0;                 // a set's q and k
    if (nc >= lim / qt || nc >= lim / N) return 0;                       // the grid's x extent; the masses (and set A's weights)
    if (nc * N >= lim / bh) return 0;                                    // the partials
    return (size_t)nc * bh * N * sizeof(float);
}

// transfer matrix (transfer_cell_kernel, transfer_cell_fold_kernel): any head dim of DSIM_FOR_EACH_D, any N, the three dtypes.
// a.q[1], a.k[0] and a.mask[0] (set A's weight bytes) are what it reads; a.v, a.q[0], a.k[1], a.mask[1] and a.similarity are not used
int launch_region_transfer_matrix(const MatrixArgs& a, int dtype, float* mass, int32_t* status, hipStream_t s) {
    if (!a.q[1] || !a.k[0] || !a.mask[0] || !mass) return DSIM_ERR_INVALID;
    const size_t need = region_transfer_matrix_scratch_bytes(a.n_a, a.n_b, a.B, a.H, a.N, a.D, dtype);
    if (need == 0) return DSIM_ERR_INVALID;
    if (a.scratch_bytes < need) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype, [&](auto e) { return launch_transfer_matrix_t<typename decltype(e)::type>(a, mass, status, s); },
        [&] { return DSIM_F16_TWIN(launch_region_transfer_matrix(a, dtype, mass, status, s)); });
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
