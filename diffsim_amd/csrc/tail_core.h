// What the score tails share on top of the tiled attention core (attn_core.h): the rounding of attend's output to the pipeline
// dtype, the products of a cross output against a self output, and a workgroup's partial.  Shared by tails.hip (pairs, maps,
// matrices) and regions.hip (region scores), which must round and multiply alike to agree bit for bit; everything here lives in
// their dsim::(anonymous namespace).
#pragma once
#include "attn_core.h"

namespace dsim {
namespace {

// ---- fused score tail ----------------------------------------------------------------------
// 16-bit modes (round 5): both SDPA outputs are rounded to the compute dtype before the products -- torch's SDPA returns
// tensors of the pipeline dtype and the reference's cosine / mse consume those (diffsim.py:177-190); the products and sums stay
// f32 per workgroup and f64 across them.  The self-attention's output then waits for the cross-attention as packed 16-bit
// pairs (40 registers at d = 160 instead of 80), which brings d = 160 from 426 registers (one workgroup per CU) under 256: two
// workgroups per CU.  The f32 parity mode keeps both outputs in f32.

// attend's output in the lane's row, rounded to the compute dtype T (the 16-bit modes convert two values at a time), folded in
// slot order: s = f(s, db, r, d, x) for every accumulator slot (db, r) whose column d is < D.  (The state goes through f by value:
// with the current compiler, sums held by reference across the walk move the register allocation of the tail kernels.)
template <typename T, int D, typename S, typename F>
__device__ __forceinline__ S fold_rounded(const OAcc<T, D>& acc, int half, S s, F&& f) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int db = 0; db < ACfg<T, D>::NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            T v[2];
            if constexpr (sizeof(T) == 2) {
                const h16x2 p = __builtin_convertvector((f32x2){acc.b[db][r], acc.b[db][r + 1]}, h16x2);
                v[0] = p[0]; v[1] = p[1];
            } else {
                v[0] = acc.b[db][r]; v[1] = acc.b[db][r + 1];
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int rr = r + e, d = db * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * half;
                if (d < D) s = f(s, db, rr, d, v[e]);
            }
        }
    return s;
}

// attend's normalised output held as plain f32 values: hipcc may otherwise fuse attend's final multiply by 1/l into what consumes
// it -- into the fp16 rounding (v_fma_mixlo_f16: one rounding instead of f32 then fp16) or into the mse difference (an fma) -- and it
// does so in some tail kernels and not in others.  Every tail calls it on every attend output, so that pair_tail_body and
// matrix_tail_kernel round and subtract the same f32 values and a matrix cell equals the pair tail's score bit for bit.
template <typename T, int D>
__device__ __forceinline__ void settle(OAcc<T, D>& acc) {
#pragma unroll
    for (int db = 0; db < ACfg<T, D>::NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (db * 32 + (r & 3) + 8 * (r >> 2) >= D) continue;      // (no lane holds a column d < D in this slot)
            float x = acc.b[db][r];
            asm volatile("" : "+v"(x));
            acc.b[db][r] = x;
        }
}

// the products of the cross output ox (rounded by fold_rounded) against the self output y(db, r, d), in f32: cosine sums
// dot | x2 | y2 into s0 | s1 | s2, mse the squared difference into s0
struct TailSums { float s0 = 0.f, s1 = 0.f, s2 = 0.f; };
template <typename T, int D, typename Y>
__device__ __forceinline__ TailSums tail_products(const OAcc<T, D>& ox, int half, int mse, Y&& y) {
    return fold_rounded<T, D>(ox, half, TailSums{}, [&](TailSums s, int db, int r, int d, T xr) {
        const float x = (float)xr, yv = y(db, r, d);
        if (mse) { const float df = x - yv; s.s0 = fmaf(df, df, s.s0); }
        else { s.s0 = fmaf(x, yv, s.s0); s.s1 = fmaf(x, x, s.s1); s.s2 = fmaf(yv, yv, s.s2); }
        return s;
    });
}

// a workgroup's products folded over its 4 waves (shuffles, then the waves in a fixed order) into its partial
// o[0..3] = (s0, s1, s2, 0); every thread of the workgroup calls it
__device__ __forceinline__ void store_block_partial(TailSums t, int lane, int wave, float* __restrict__ o) {
    __shared__ float red[4][4];
    float s0 = t.s0, s1 = t.s1, s2 = t.s2;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_xor(s0, off);
        s1 += __shfl_xor(s1, off);
        s2 += __shfl_xor(s2, off);
    }
    if (lane == 0) { red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        o[0] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
        o[1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
        o[2] = (red[0][2] + red[1][2]) + (red[2][2] + red[3][2]);
        o[3] = 0.f;
    }
}

}  // namespace
}  // namespace dsim
