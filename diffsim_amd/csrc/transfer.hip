// Region transfer: the attention mass a token sends into the other image's weighted tokens.  With Pm the token alignments' attention
// (align_core.h: P_bh = softmax over ALL keys of the un-rescaled logits, the scale entering in f32, Pm its mean over the B CFG halves
// and the H heads) and w_x[j] = byte / 255 the key image's token weights,
//   mass[p][0][i] = sum_j Pm_ab[i][j] w_b[j]   (a's queries over b's keys),   mass[p][1][u] = sum_t Pm_ba[u][t] w_a[t]   (the mirror).
// The weights enter the sum only: no bias joins the logits (unlike the soft tails) and the softmax is the alignments'.  Pm is never
// formed: sum_j Pm[i][j] w[j] = mean over (b, h) of (sum_j e_ij w_j) / (sum_j e_ij), so one pass over the keys with two running sums
// per query row serves, and there is no statistics pass.
//
// Work layout.  The per-(b, h) partials go through a workspace with a fixed-order fold behind them (rather than one workgroup walking
// all B H steps): a chunk of a few pairs still fills the chip, and a (b, h) step keeps one Q fragment set for all its key tiles.
//   transfer_part_kernel   one workgroup per (query tile of 128, b h, pair and direction): the logits of a 64-key tile from
//                          align_logits (the alignments' MFMA sequence on the same operands, staged by align_k_load / align_k_store),
//                          the online maximum m, and per lane half the two f32 sums l = sum_j e_ij and num = sum_j fmaf(e_ij, w_j, .)
//                          with e_ij = exp2(fma(s, c, -m c)); per tile the sums start at 0 and join the running ones as
//                          fmaf(running, alpha, tile), both rescaled by the same alpha when the maximum moves.  r_bh = num / l
//                          (the halves added lower first) is the one value stored: part[pair][dir][bh][N] f32, the whole workspace.
//   transfer_fold_kernel   one thread per output element: mass = (sum over bh ascending of r_bh) * (1 / (B H)), and status[pair] = 1
//                          (a plain store into a word the launcher zeroed) where that is not finite.
// The key weights of a tile reach the lanes once per tile: 64 threads convert the tile's bytes (w = (float)byte / 255.0f, 0 past the
// end) a tile ahead, beside the K chunks, and store them next to the K tile in LDS; a lane reads its 32 as eight 16-byte LDS loads.
// No atomics, one writer per element; a row's value depends on its query row, its key image's rows and weights and nothing else: not
// on the call's other pairs, the directions asked for or other images' weights.  Rows of a direction not asked for are not written.
#include "align_core.h"

namespace dsim {
namespace {

// grid (ceil(N/128), B*H, n_pairs * (directions == 3 ? 2 : 1))
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void transfer_part_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                               const uint8_t* __restrict__ wg, const int32_t* __restrict__ idx_a,
                                                               const int32_t* __restrict__ idx_b, int B, int H, int N, float c,
                                                               int directions, float* __restrict__ part) {
    typedef ACfg<T, D> C;
    __shared__ __attribute__((aligned(16))) char lds[C::TILEK];
    __shared__ __attribute__((aligned(16))) float wl[KT];        // the tile's key weights; 0 past the end
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
    const int pair = directions == 3 ? (int)blockIdx.z >> 1 : (int)blockIdx.z, dir = directions == 3 ? (int)blockIdx.z & 1 : directions - 1;
    const int ia = idx_a[pair], ib = idx_b[pair];
    const int iq = dir ? ib : ia, ix = dir ? ia : ib;
    const int ld = H * D;
    const size_t img = (size_t)B * N * ld, boff = (size_t)b * N * ld + h * D;
    const int q = blockIdx.x * 128 + wave * 32 + l31;                // query position (past the end: the last one's row)
    const int qc = q < N ? q : N - 1;
    QFrags<T, D> qf;
    align_load_q<T, D>(qf, qg + iq * img + boff + (size_t)qc * ld, half);
    const T* kb = kg + ix * img + boff;
    const uint8_t* wb = wg + (size_t)ix * N;
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
    if (half == 0 && q < N) part[(((size_t)pair * 2 + dir) * gridDim.y + bh) * N + q] = num / l;
}

// one thread per (pair, direction asked for, token)
__global__ __launch_bounds__(256) void transfer_fold_kernel(const float* __restrict__ part, int n_pairs, int BH, int N, float rbh,
                                                            int directions, float* __restrict__ mass, int32_t* __restrict__ status) {
    const int nd = directions == 3 ? 2 : 1;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)n_pairs * nd * N) return;
    const int i = (int)(t % N);
    const size_t z = t / N;
    const int pair = (int)(z / nd), dir = directions == 3 ? (int)(z & 1) : directions - 1;
    const size_t row = (size_t)pair * 2 + dir;
    const float* p = part + row * BH * N + i;
    float total = 0.f;
    for (int bh = 0; bh < BH; ++bh) total += p[(size_t)bh * N];
    const float v = total * rbh;
    mass[row * N + i] = v;
    // (the exponent bits, not v - v == 0: v is a product, and contracted into an fma with it that difference is the product's rounding
    // error, non-zero for a finite v whenever 1 / (B H) is no power of two)
    if (status && (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) status[pair] = 1;
}

template <typename T>
int launch_transfer_t(const PairArgs& a, const uint8_t* weights, int directions, float* mass, int32_t* status, hipStream_t s) {
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value;
        const int qt = (a.N + 127) / 128, nd = directions == 3 ? 2 : 1, BH = a.B * a.H;
        if (status) DSIM_HIP_CHECK(hipMemsetAsync(status, 0, (size_t)a.n_pairs * sizeof(int32_t), s));
        hipLaunchKernelGGL((transfer_part_kernel<T, Dc>), dim3(qt, BH, a.n_pairs * nd), dim3(256), 0, s, (const T*)a.q, (const T*)a.k, weights,
                           a.idx_a, a.idx_b, a.B, a.H, a.N, scale_log2_of(Dc), directions, (float*)a.scratch);
        DSIM_HIP_CHECK(hipGetLastError());
        const size_t total = (size_t)a.n_pairs * nd * a.N;
        hipLaunchKernelGGL(transfer_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)a.scratch, a.n_pairs, BH,
                           a.N, 1.0f / (float)BH, directions, mass, status);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
// the partials of transfer_part_kernel, [pair][dir][bh][N] f32; 0 for a call the launcher does not serve for its shape
size_t pair_region_transfer_scratch_bytes(int n_feat, int n_pairs, int B, int H, int N, int D) {
    if (!pair_shape_served(n_pairs, B, H, N, D)) return 0;
    if (n_feat < 1 || (size_t)n_feat * N >= ((size_t)1 << 31)) return 0;
    return (size_t)n_pairs * 2 * B * H * N * sizeof(float);
}

// region transfer (transfer_part_kernel, transfer_fold_kernel): any head dim of DSIM_FOR_EACH_D, any N, the three dtypes (a.v and
// a.similarity are not used)
int launch_pair_region_transfer(const PairArgs& a, int dtype, const uint8_t* weights, int n_feat, int directions, float* mass,
                                int32_t* status, hipStream_t s) {
    const int st = pair_args_check(a, dtype);
    if (st != DSIM_OK) return st;
    if (directions < 1 || directions > 3 || !weights || !mass) return DSIM_ERR_INVALID;
    const size_t need = pair_region_transfer_scratch_bytes(n_feat, a.n_pairs, a.B, a.H, a.N, a.D);
    if (need == 0) return DSIM_ERR_INVALID;
    if (a.scratch_bytes < need) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype, [&](auto e) { return launch_transfer_t<typename decltype(e)::type>(a, weights, directions, mass, status, s); },
        [&] { return DSIM_F16_TWIN(launch_pair_region_transfer(a, dtype, weights, n_feat, directions, mass, status, s)); });
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
