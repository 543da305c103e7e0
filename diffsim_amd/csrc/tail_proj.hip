// The projected score tail: the DiffSim pair tail with the hooked layer's output projection between the attentions and the cosine
// -- the reference's CLIPScore.attention_calc (metrics/clip_i.py:143-159):
//     P_xy = out_proj(SDPA(q_x, k_y, v_y)) as [B][N][C] rows, C = H D, bias included;  score = 1/2 [cos(P_ab, P_aa) + cos(P_ba, P_bb)]
// The projection mixes the heads, so the attention outputs cannot stay in one workgroup's registers as tails.hip's do: they go
// through a workspace slab.
//  * proj_attend_kernel:   one attention per (pair, direction, cross | self, b, h, 128 queries) on the tiled core (attn_core.h's
//                          attend, tail_core.h's settle and fold_rounded: the pair tail's arithmetic and rounding), O into the slab
//                          [pair][dir][cross | self][B][N][C] in the compute dtype.
//  * proj_products_kernel: PR rows of a (pair, direction) per workgroup: both O row blocks staged in LDS as f32, one output feature
//                          per thread and pass -- P = O W^T + b by f32 fmaf over k in ascending order, rounded to the compute
//                          dtype -- then the pair tail's products (tail_products' arithmetic) and store_block_partial.
//  * pair_finish_kernel (tail_core.h): the f64 fold in a fixed order, eps 1e-8, mse over B N C values.
// No atomics; a pair's workgroups read and write only that pair's slab rows and partials, so a score is bit-identical alone and in a
// batch.  Compiled once per 16-bit type; the C entry points live in the bf16 object.
#include "tail_core.h"

namespace dsim {

// this source's own host entry points, per 16-bit type as h16_api.h's (declared here: no other source calls them)
inline namespace DSIM_H16_NS {
size_t pair_score_proj_scratch_bytes(int n_pairs, int B, int H, int N, int D, int dtype);      // 0: call not served
int launch_pair_score_proj(const PairArgs& a, int dtype, const void* w_out, const float* bias, float* out, int32_t* status, hipStream_t s);
}
#if !defined(DSIM_H16_IS_F16) && !defined(DSIM_DEVTOOLS)
namespace f16 {
size_t pair_score_proj_scratch_bytes(int n_pairs, int B, int H, int N, int D, int dtype);
int launch_pair_score_proj(const PairArgs& a, int dtype, const void* w_out, const float* bias, float* out, int32_t* status, hipStream_t s);
}
#endif

namespace {

constexpr int PR = 8;               // rows of a (pair, direction) per products workgroup
constexpr int PROJ_MAX_C = 1024;    // 2 PR rows of C f32 values in LDS: 64 KB

// grid (ceil(N/128), B*H*2, n_pairs*2): y = (b, h, cross | self), z = (pair, direction)
template <typename T, int D>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void proj_attend_kernel(const T* __restrict__ qg, const T* __restrict__ kg,
                                                          const T* __restrict__ vg, const int32_t* __restrict__ idx_a,
                                                          const int32_t* __restrict__ idx_b, int B, int H, int N,
                                                          float scale_log2, T* __restrict__ slab) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int self = blockIdx.y & 1, bh = blockIdx.y >> 1, b = bh / H, h = bh - b * H;
    const int pair = blockIdx.z >> 1, dir = blockIdx.z & 1;
    const int ia = idx_a[pair], ib = idx_b[pair];
    const int iq = dir ? ib : ia;                  // query image
    const int ikv = self ? iq : (dir ? ia : ib);   // key / value image
    const int ld = H * D;
    const size_t img = (size_t)B * N * ld;
    const size_t boff = (size_t)b * N * ld + h * D;
    const int t = blockIdx.x * 128 + wave * 32 + l31;          // query position
    const int q = t < N ? t : N - 1;                           // its row (a position past the end: the last one's)
    QFrags<T, D> qf;
    load_q<T, D>(qf, qg + iq * img + boff + (size_t)q * ld, half, scale_log2);
    OAcc<T, D> oa;
    attend<T, D, false>(qf, kg + ikv * img + boff, vg + ikv * img + boff, ld, N, smem, oa);
    settle<T, D>(oa);
    T* so = slab + (((size_t)pair * 2 + dir) * 2 + self) * img + boff;
    if (t < N) fold_rounded<T, D>(oa, half, 0, [&](int, int, int, int d, T y) { so[(size_t)t * ld + d] = y; return 0; });      // (no state)
}

// grid (ceil(rows / PR), n_pairs*2), rows = B*N; dynamic LDS 2 * PR * C floats
template <typename T>
__global__ __launch_bounds__(256) void proj_products_kernel(const T* __restrict__ slab, const T* __restrict__ w, const float* __restrict__ bias,
                                                            int rows, int C, int mse, float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* ol = (float*)smem;                                  // [2 (cross | self)][PR][C]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pd = blockIdx.y, r0 = blockIdx.x * PR;
    const T* base = slab + (size_t)pd * 2 * rows * C;
    for (int i = threadIdx.x; i < 2 * PR * C; i += 256) {
        const int sr = i / C, c = i - sr * C, which = sr / PR, r = r0 + (sr - which * PR);
        ol[i] = r < rows ? (float)base[((size_t)which * rows + r) * C + c] : 0.f;
    }
    __syncthreads();
    constexpr int VEC = 16 / sizeof(T);
    typedef T VecT __attribute__((ext_vector_type(VEC)));
    TailSums s;
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc[2 * PR];
#pragma unroll
        for (int r = 0; r < 2 * PR; ++r) acc[r] = 0.f;
        const T* wr = w + (size_t)c * C;
        for (int k0 = 0; k0 < C; k0 += VEC) {
            const VecT wv = *(const VecT*)(wr + k0);
#pragma unroll
            for (int j0 = 0; j0 < VEC; j0 += 4) {
#pragma unroll
                for (int r = 0; r < 2 * PR; ++r) {
                    const f32x4 o4 = *(const f32x4*)(ol + (size_t)r * C + k0 + j0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[r] = fmaf(o4[j], (float)wv[j0 + j], acc[r]);
                }
            }
        }
        const float bv = bias[c];
#pragma unroll
        for (int r = 0; r < PR; ++r) {
            if (r0 + r >= rows) continue;
            const float x = (float)(T)(acc[r] + bv), y = (float)(T)(acc[PR + r] + bv);
            if (mse) { const float df = x - y; s.s0 = fmaf(df, df, s.s0); }
            else { s.s0 = fmaf(x, y, s.s0); s.s1 = fmaf(x, x, s.s1); s.s2 = fmaf(y, y, s.s2); }
        }
    }
    store_block_partial(s, lane, wave, part + ((size_t)pd * gridDim.x + blockIdx.x) * 4);
}

// workspace: the O slab | partials f32 [n_pairs][2][row tiles][4], each 256-byte aligned
struct ProjLayout {
    size_t slab, parts;
    int nrt;
    ProjLayout(int n_pairs, int B, int H, int N, int D, size_t es) {
        nrt = (B * N + PR - 1) / PR;
        slab = up256((size_t)n_pairs * 4 * B * N * H * D * es);
        parts = up256((size_t)n_pairs * 2 * nrt * 4 * sizeof(float));
    }
    size_t total() const { return slab + parts; }
};

bool proj_served(const PairArgs& a, int dtype) {
    if (pair_args_check(a, dtype) != DSIM_OK) return false;
    if ((long)a.B * a.H * 2 > 65535 || (long)a.H * a.D > PROJ_MAX_C) return false;
    return ((long)a.B * a.N + PR - 1) / PR <= 0x7fffffffl;
}

template <typename T>
int launch_proj_t(const PairArgs& a, const void* w_out, const float* bias, float* out, int32_t* status, hipStream_t s) {
    const ProjLayout L(a.n_pairs, a.B, a.H, a.N, a.D, sizeof(T));
    T* slab = (T*)a.scratch;
    float* part = (float*)((char*)a.scratch + L.slab);
    const int C = a.H * a.D;
    return with_head_dim(a.D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value, LDS = ACfg<T, Dc>::LDS;
        int st = launch_lds<proj_attend_kernel<T, Dc>>(dim3((a.N + 127) / 128, a.B * a.H * 2, a.n_pairs * 2), dim3(256), LDS, s, (const T*)a.q,
                                                       (const T*)a.k, (const T*)a.v, a.idx_a, a.idx_b, a.B, a.H, a.N, scale_log2_of(Dc), slab);
        if (st != DSIM_OK) return st;
        st = launch_lds<proj_products_kernel<T>>(dim3(L.nrt, a.n_pairs * 2), dim3(256), 2 * PR * PROJ_MAX_C * (int)sizeof(float), s,
                                                 (const T*)slab, (const T*)w_out, bias, a.B * a.N, C, a.similarity, part);
        if (st != DSIM_OK) return st;
        return launch_pair_finish<false>(part, nullptr, nullptr, nullptr, a.n_pairs, L.nrt, a.similarity, (double)a.B * a.N * C, out, status, s);
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
size_t pair_score_proj_scratch_bytes(int n_pairs, int B, int H, int N, int D, int dtype) {
    PairArgs a;
    a.n_pairs = n_pairs; a.B = B; a.H = H; a.N = N; a.D = D;
    if (!proj_served(a, dtype)) return 0;
    return ProjLayout(n_pairs, B, H, N, D, dtype_size(dtype)).total();
}

int launch_pair_score_proj(const PairArgs& a, int dtype, const void* w_out, const float* bias, float* out, int32_t* status, hipStream_t s) {
    if (!proj_served(a, dtype)) return DSIM_ERR_INVALID;
    if (a.scratch_bytes < pair_score_proj_scratch_bytes(a.n_pairs, a.B, a.H, a.N, a.D, dtype)) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype, [&](auto e) { return launch_proj_t<typename decltype(e)::type>(a, w_out, bias, out, status, s); },
        [&] { return DSIM_F16_TWIN(launch_pair_score_proj(a, dtype, w_out, bias, out, status, s)); });
}
}  // namespace DSIM_H16_NS

}  // namespace dsim

#ifndef DSIM_H16_IS_F16
using namespace dsim;

extern "C" {

size_t dsim_pair_score_proj_workspace_bytes(int n_pairs, int B, int H, int N, int D, int dtype) {
    const size_t b = pair_score_proj_scratch_bytes(n_pairs, B, H, N, D, dtype);
    return b ? b + 256 : 0;
}

int dsim_pair_score_proj(const void* q, const void* k, const void* v, const int32_t* idx_a, const int32_t* idx_b, int n_pairs, int B, int H,
                         int N, int D, int dtype, int similarity, const void* w_out, const float* bias, float* out_scores, int32_t* status,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!q || !k || !v || !idx_a || !idx_b || !w_out || !bias || !out_scores || !workspace) return DSIM_ERR_INVALID;
    PairArgs a{q, k, v, idx_a, idx_b, n_pairs, B, H, N, D, similarity, workspace, workspace_bytes};
    if (pair_score_proj_scratch_bytes(n_pairs, B, H, N, D, dtype) == 0 || (similarity != 0 && similarity != 1)) return DSIM_ERR_INVALID;
    const size_t lost = (size_t)(-(uintptr_t)workspace & 255);      // the workspace starts at its first 256-byte boundary
    if (workspace_bytes < lost) return DSIM_ERR_WORKSPACE;
    a.scratch = (char*)workspace + lost;
    a.scratch_bytes = workspace_bytes - lost;
    return launch_pair_score_proj(a, dtype, w_out, bias, out_scores, status, (hipStream_t)stream);
}

}  // extern "C"
#endif
