// What the per-token region forms share besides the two cores: the kernel that writes the alignments' off values, the workspace
// layout in front of a call's partials or statistics, and the shape check.  Shared by region_maps.hip (region maps and alignments)
// and soft_maps.hip (their soft forms); in their dsim::(anonymous namespace).
#pragma once
#include "align_core.h"
#include "tail_core.h"

namespace dsim {
namespace {

// One workgroup per (pair, direction): the off values at the rows region_align_kernel does not write -- the off query tokens, and
// every token when an image of the pair is empty -- and, from direction 0's first thread, the pair's status word.  Together with
// region_align_kernel every element of match, weight and expect has one writer.
constexpr int OFF_THREADS = 256;
__global__ __launch_bounds__(OFF_THREADS) void region_align_off_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ cnt,
                                                                       const int32_t* __restrict__ idx_a, const int32_t* __restrict__ idx_b,
                                                                       int N, int32_t* __restrict__ match, float* __restrict__ weight,
                                                                       float* __restrict__ expect, int32_t* __restrict__ status) {
    const int pd = blockIdx.x, pair = pd >> 1, dir = pd & 1;
    const int ia = idx_a[pair], ib = idx_b[pair];
    const bool empty = cnt[ia] == 0 || cnt[ib] == 0;
    const uint8_t* m = mask + (size_t)(dir ? ib : ia) * N;
    for (int i = threadIdx.x; i < N; i += OFF_THREADS) {
        if (!empty && m[i] != 0) continue;
        const size_t o = (size_t)pd * N + i;
        if (match) match[o] = -1;
        if (weight) weight[o] = 0.f;
        if (expect) *reinterpret_cast<float2*>(expect + 2 * o) = make_float2(-1.f, -1.f);
    }
    if (status && dir == 0 && threadIdx.x == 0) status[pair] = empty ? 2 : 0;
}

// workspace: [lists int32 [n_feat][N] | counts int32 [n_feat] | the call's partials or statistics], each 256-byte aligned
struct RegionLayout {
    size_t lists, counts;
    RegionLayout(int n_feat, int N) : lists(up256((size_t)n_feat * N * sizeof(int32_t))), counts(up256((size_t)n_feat * sizeof(int32_t))) {}
    int32_t* list(void* ws) const { return (int32_t*)ws; }
    int32_t* cnt(void* ws) const { return (int32_t*)((char*)ws + lists); }
    void* rest(void* ws) const { return (char*)ws + lists + counts; }
};
bool region_call_served(int n_feat, int n_pairs, int B, int H, int N, int D) {
    return n_feat >= 1 && pair_shape_served(n_pairs, B, H, N, D) && (long)n_feat * N < (1l << 31);
}

}  // namespace
}  // namespace dsim
