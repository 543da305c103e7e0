// What the soft region forms share on top of the score tails (tail_core.h): the bias table, the kernel that turns an image's weight
// bytes into key biases and a byte sum, the workspace sizes of both, and the finish that takes the mse count from the byte sums.
// Shared by soft_regions.hip (soft region scores) and soft_matrix.hip (soft score matrices), which must bias and count alike to
// agree bit for bit; everything here lives in their dsim::(anonymous namespace).
#pragma once
#include <cmath>

#include "tail_core.h"

namespace dsim {
namespace {

constexpr int SOFT_THREADS = 256;

struct BiasTable { float v[256]; };

// log2(m / 255) in double, rounded once to f32; entry 0 is never read (a byte 0 is not listed)
const BiasTable& bias_table() {
    static const BiasTable t = [] {
        BiasTable b;
        b.v[0] = -INFINITY;
        for (int m = 1; m < 256; ++m) b.v[m] = (float)std::log2((double)m / 255.0);
        return b;
    }();
    return t;
}

// One workgroup per feature image: lb[img][j] = tab[m[list[j]]] for j < count, 0 from there to the row's end (stride: N rounded up
// to whole key tiles, so attend's loads of a ragged tile stay inside the row; those logits are masked after the addition), and
// sum[img] = the image's byte sum (also to sums_out when the caller asked).  Integer sums: the order does not matter.
__global__ __launch_bounds__(SOFT_THREADS) void soft_weights_kernel(const BiasTable tab, const uint8_t* __restrict__ w, int N, int stride,
                                                                    const int32_t* __restrict__ list, const int32_t* __restrict__ cnt,
                                                                    float* __restrict__ lb, int32_t* __restrict__ sum,
                                                                    int32_t* __restrict__ sums_out) {
    __shared__ int wtot[SOFT_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* m = w + (size_t)blockIdx.x * N;
    const int32_t* l = list + (size_t)blockIdx.x * N;
    float* o = lb + (size_t)blockIdx.x * stride;
    const int n = cnt[blockIdx.x];
    for (int j = tid; j < stride; j += SOFT_THREADS) o[j] = j < n ? tab.v[m[l[j]]] : 0.f;
    int acc = 0;
    for (int t = tid; t < N; t += SOFT_THREADS) acc += m[t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) wtot[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int i = 0; i < SOFT_THREADS / 64; ++i) total += wtot[i];
        sum[blockIdx.x] = total;
        if (sums_out) sums_out[blockIdx.x] = total;
    }
}

// One thread per pair: pair_finish_kernel<true>'s fold with the directions' mse counts from the byte sums, count = B H D, the
// elements per row, times (sum of the query image's bytes) / 255 in f64; a pair with an image of byte sum 0: NaN and status 2.
__global__ void soft_finish_kernel(const float* __restrict__ part, const int32_t* __restrict__ sum, const int32_t* __restrict__ idx_a,
                                   const int32_t* __restrict__ idx_b, int n_pairs, int nblk, int mse, double count,
                                   float* __restrict__ out, int32_t* __restrict__ status) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const int n[2] = {sum[idx_a[p]], sum[idx_b[p]]};
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
        res += direction_value(a, x2, y2, mse, count * ((double)n[dir] / 255.0));
    }
    store_score(res, out + p, status ? status + p : nullptr);
}

// the biases' row stride and the sizes of the soft forms' own workspace parts, each 256-byte aligned
int soft_stride(int N) { return (N + KT - 1) / KT * KT; }
size_t soft_list_bytes(int n_feat, int N) { return up256((size_t)n_feat * N * sizeof(int32_t)); }
size_t soft_count_bytes(int n_feat) { return up256((size_t)n_feat * sizeof(int32_t)); }
size_t soft_bias_bytes(int n_feat, int N) { return up256((size_t)n_feat * soft_stride(N) * sizeof(float)); }

}  // namespace
}  // namespace dsim
