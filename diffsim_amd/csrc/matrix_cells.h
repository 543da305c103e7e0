// The cells of a listed score matrix among its n_a + n_b row lists: what a pair finish reads a cell's two images through.  Shared by
// region_matrix.hip and soft_matrix.hip; in their dsim::(anonymous namespace).
#pragma once
#include "tail_core.h"

namespace dsim {
namespace {

// idx_a[c] = c / n_b, idx_b[c] = n_a + c % n_b: set A's images at index i, set B's at n_a + j
__global__ void cell_index_kernel(int n_a, int n_b, int32_t* __restrict__ idx_a, int32_t* __restrict__ idx_b) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_a * n_b) return;
    idx_a[c] = c / n_b;
    idx_b[c] = n_a + c % n_b;
}

}  // namespace
}  // namespace dsim
