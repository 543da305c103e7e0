// Region scores: the DiffSim score tail restricted to a token region per image.  Every feature image i carries a region
// R_i of its N tokens (a byte mask, non-zero = on); the region score of (a, b) is the reference's tail -- diffsim/diffsim.py:177-197 --
// on the sub-tensors Q_a[R_a], K_a[R_a], V_a[R_a] and Q_b[R_b], K_b[R_b], V_b[R_b], rows in ascending token order: the off tokens are
// neither queries nor keys, so they take part in no softmax.  With every region full it is the pair score.
//
//   region_lists_kernel   the masks as ascending token lists and counts (the workspace)
//   region_tail_kernel    pair_tail_kernel's arithmetic (tails.hip: attend twice on one set of Q fragments, the rounding, the
//                         products, the partial layout) with the rows taken through the lists: compacted position t of an image is
//                         its row list[t], and the image's count stands where N stood
//   region_finish_kernel  pair_finish_kernel's fixed-order f64 fold, the direction's own element count for mse, and an empty
//                         region reported instead of scored
// The kernels live here, not in tails.hip: the region tail is one more instantiation of attend per head dim and dtype, and in its
// own source it cannot move the register allocation or the code of the pair, map and matrix tails.
#include "tail_core.h"

namespace dsim {
namespace {

constexpr int LIST_THREADS = 256;

// One workgroup per feature image: list[img][0 .. count) = the on tokens ascending, cnt[img] = count (also to counts_out when the
// caller asked).  256 tokens a round: a ballot per wave, the lane's rank from the lower lanes' bits, the waves' totals through LDS.
// Every entry has one writer; the entries from count on are not written and never read.
__global__ __launch_bounds__(LIST_THREADS) void region_lists_kernel(const uint8_t* __restrict__ mask, int N, int32_t* __restrict__ list,
                                                                    int32_t* __restrict__ cnt, int32_t* __restrict__ counts_out) {
    __shared__ int wtot[LIST_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* m = mask + (size_t)blockIdx.x * N;
    int32_t* out = list + (size_t)blockIdx.x * N;
    int base = 0;
    for (int t0 = 0; t0 < N; t0 += LIST_THREADS) {
        const int t = t0 + tid;
        const bool on = t < N && m[t] != 0;
        const unsigned long long bits = __ballot(on);
        const int rank = __popcll(bits & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wave] = __popcll(bits);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < LIST_THREADS / 64; ++w) {
            if (w < wave) before += wtot[w];
            total += wtot[w];
        }
        if (on) out[base + before + rank] = t;
        base += total;
        __syncthreads();                   // (wtot is read before the next round writes it)
    }
    if (tid == 0) {
        cnt[blockIdx.x] = base;
        if (counts_out) counts_out[blockIdx.x] = base;
    }
}

// One direction of a pair in a workgroup of 128 compacted query positions: pair_tail_body (tails.hip) with listed rows.
// grid (ceil(N/128), B*H, n_pairs*2): the worst case, the counts being on the device; a workgroup past the query region's end, or of
// a pair with an empty region, writes a zero partial and leaves as a whole before any barrier.  part: [pair][dir][bh][qtile][4] f32
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void region_tail_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                        const T* __restrict__ vg, const int32_t* __restrict__ list,
                                                        const int32_t* __restrict__ cnt, const int32_t* __restrict__ idx_a,
                                                        const int32_t* __restrict__ idx_b, int B, int H, int N,
                                                        float scale_log2, int mse, float* __restrict__ part) {
    typedef ACfg<T, D> C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
    const int pair = blockIdx.z >> 1, dir = blockIdx.z & 1;
    const int ia = idx_a[pair], ib = idx_b[pair];
    const int iq = dir ? ib : ia;        // query image (also the "self" keys/values)
    const int ix = dir ? ia : ib;        // the other image ("cross" keys/values)
    const int nq = cnt[iq], nx = cnt[ix];
    float* const o = part + ((((size_t)pair * 2 + dir) * gridDim.y + bh) * gridDim.x + blockIdx.x) * 4;
    if ((int)blockIdx.x * 128 >= nq || nx == 0) {          // (uniform over the workgroup)
        if (threadIdx.x == 0) o[0] = o[1] = o[2] = o[3] = 0.f;
        return;
    }
    const RowsListed rq = {list + (size_t)iq * N}, rx = {list + (size_t)ix * N};
    const int ld = H * D;
    const size_t img = (size_t)B * N * ld;
    const int t = blockIdx.x * 128 + wave * 32 + l31;      // compacted query position
    const int q = rq.list[t < nq ? t : nq - 1];            // its row
    const size_t boff = (size_t)b * N * ld + h * D;
    QFrags<T, D> qf;
    load_q<T, D>(qf, qg + iq * img + boff + (size_t)q * ld, half, scale_log2);
    TailSums s;
    if constexpr (sizeof(T) == 2) {
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        h16x2 osp[C::NDB][8];           // the self-attention's output, rounded to the compute dtype, two values per register
        {
            OAcc<T, D> osa;
            attend<T, D, false>(qf, kg + iq * img + boff, vg + iq * img + boff, ld, nq, smem, osa, nullptr, rq);
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
        attend<T, D, false>(qf, kg + ix * img + boff, vg + ix * img + boff, ld, nx, smem, oxa, nullptr, rx);
        settle<T, D>(oxa);
        if (t < nq) s = tail_products<T, D>(oxa, half, mse, [&](int db, int r, int) { return (float)osp[db][r >> 1][r & 1]; });
    } else {
        OAcc<T, D> osa, oxa;
        attend<T, D, false>(qf, kg + iq * img + boff, vg + iq * img + boff, ld, nq, smem, osa, nullptr, rq);
        attend<T, D, false>(qf, kg + ix * img + boff, vg + ix * img + boff, ld, nx, smem, oxa, nullptr, rx);
        settle<T, D>(osa);
        settle<T, D>(oxa);
        if (t < nq) s = tail_products<T, D>(oxa, half, mse, [&](int db, int r, int) { return osa.b[db][r]; });
    }
    store_block_partial(s, lane, wave, o);
}

// one thread per pair: pair_finish_kernel's fold (the partials of the workgroups that left are zeros), mse over the direction's
// own B H |R_q| D elements; a pair with an empty region: NaN and status 2
__global__ void region_finish_kernel(const float* __restrict__ part, const int32_t* __restrict__ cnt, const int32_t* __restrict__ idx_a,
                                     const int32_t* __restrict__ idx_b, int n_pairs, int nblk, int mse, double per_row,
                                     float* __restrict__ out, int32_t* __restrict__ status) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const int n[2] = {cnt[idx_a[p]], cnt[idx_b[p]]};
    if (n[0] == 0 || n[1] == 0) {
        out[p] = __builtin_nanf("");
        if (status) status[p] = 2;
        return;
    }
    double res = 0.0;
    for (int dir = 0; dir < 2; ++dir) {
        double a = 0.0, x2 = 0.0, y2 = 0.0;
        const float* o = part + ((size_t)p * 2 + dir) * nblk * 4;
        for (int i = 0; i < nblk; ++i) { a += o[4 * i]; x2 += o[4 * i + 1]; y2 += o[4 * i + 2]; }
        if (mse) res += a / (per_row * n[dir]);
        else {
            const double nx = sqrt(x2), ny = sqrt(y2);
            res += a / (fmax(nx, 1e-8) * fmax(ny, 1e-8));
        }
    }
    const float sc = (float)(res * 0.5);
    out[p] = sc;
    if (status) status[p] = (sc - sc == 0.0f) ? 0 : 1;
}

// workspace: [lists int32 [n_feat][N] | counts int32 [n_feat] | partials f32 [n_pairs][2][B H][qtiles][4]], each 256-byte aligned
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
size_t region_list_bytes(int n_feat, int N) { return up256((size_t)n_feat * N * sizeof(int32_t)); }
size_t region_count_bytes(int n_feat) { return up256((size_t)n_feat * sizeof(int32_t)); }

template <typename T>
int launch_regions_t(const void* q, const void* k, const void* v, const uint8_t* mask, int n_feat, const int32_t* ia, const int32_t* ib,
                     int n_pairs, int B, int H, int N, int D, int mse, float* out, int32_t* status, int32_t* counts, void* scratch,
                     hipStream_t s) {
    int32_t* list = (int32_t*)scratch;
    int32_t* cnt = (int32_t*)((char*)scratch + region_list_bytes(n_feat, N));
    float* part = (float*)((char*)cnt + region_count_bytes(n_feat));
    return with_head_dim(D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        const int qt = (N + 127) / 128;
        hipLaunchKernelGGL(region_lists_kernel, dim3(n_feat), dim3(LIST_THREADS), 0, s, mask, N, list, cnt, counts);
        DSIM_HIP_CHECK(hipGetLastError());
        const int st = launch_lds<region_tail_kernel<T, Dc>>(dim3(qt, B * H, n_pairs * 2), dim3(256), LDS, s, (const T*)q, (const T*)k,
                                                             (const T*)v, (const int32_t*)list, (const int32_t*)cnt, ia, ib, B, H, N,
                                                             scale_log2_of(Dc), mse, part);
        if (st != DSIM_OK) return st;
        hipLaunchKernelGGL(region_finish_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, s, (const float*)part, (const int32_t*)cnt, ia,
                           ib, n_pairs, qt * B * H, mse, (double)B * H * Dc, out, status);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
// 0 for a call launch_pair_score_regions refuses for its shape
size_t pair_score_regions_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    if (n_feat < 1 || n_pairs < 1 || B < 1 || H < 1 || N < 1) return 0;
    if (n_pairs * 2 > 65535 || B * H > 65535 || (long)n_feat * N >= (1l << 31)) return 0;
    if (with_head_dim(D, [](auto) { return DSIM_OK; }) != DSIM_OK) return 0;
    return region_list_bytes(n_feat, N) + region_count_bytes(n_feat) + up256((size_t)n_pairs * 2 * B * H * ((N + 127) / 128) * 4 * sizeof(float));
}

// region scores (region_lists_kernel, region_tail_kernel, region_finish_kernel): any head dim of DSIM_FOR_EACH_D, any N, the three
// dtypes; the default tap runs the tiled kernel too
int launch_pair_score_regions(const void* q, const void* k, const void* v, const uint8_t* mask, int n_feat, const int32_t* ia,
                              const int32_t* ib, int n_pairs, int B, int H, int N, int D, int dtype, int similarity, float* out,
                              int32_t* status, int32_t* counts, void* scratch, size_t scratch_bytes, hipStream_t s) {
    if (dtype != DSIM_F32 && dtype != DSIM_BF16 && dtype != DSIM_F16) return DSIM_ERR_INVALID;
    if (similarity != 0 && similarity != 1) return DSIM_ERR_INVALID;
    const size_t need = pair_score_regions_scratch_bytes(n_feat, n_pairs, B, H, N, D);
    if (need == 0) return DSIM_ERR_INVALID;
    if (scratch_bytes < need) return DSIM_ERR_WORKSPACE;
    if (dtype == DSIM_H16)
        return launch_regions_t<h16>(q, k, v, mask, n_feat, ia, ib, n_pairs, B, H, N, D, similarity, out, status, counts, scratch, s);
#ifndef DSIM_H16_IS_F16
    if (dtype == DSIM_F32)
        return launch_regions_t<float>(q, k, v, mask, n_feat, ia, ib, n_pairs, B, H, N, D, similarity, out, status, counts, scratch, s);
    if (dtype == DSIM_F16)
        return DSIM_F16_TWIN(launch_pair_score_regions(q, k, v, mask, n_feat, ia, ib, n_pairs, B, H, N, D, dtype, similarity, out, status,
                                                       counts, scratch, scratch_bytes, s));
#endif
    return DSIM_ERR_INVALID;
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
