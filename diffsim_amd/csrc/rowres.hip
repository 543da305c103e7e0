// Row-resident transformer kernels for the 320-channel (64 x 64) level of the SD U-Net, gfx950, h16.
//
// The BasicTransformerBlock's feed-forward at C = 320 -- LayerNorm -> Linear(C, 8C) -> h * gelu(g) -> Linear(4C, C) ->
// + residual (control flow: /root/reference/diffsim/hacked_modules.py:82-132, the diffusers FeedForward / GEGLU modules
// behind it) -- is ONE kernel here.  As three launches it moved the 4C-wide intermediate through HBM twice (1.34 GB
// written + 1.34 GB read per layer at 32 pairs) and spent as long in the erf-GELU epilogue as in the MFMAs.
//
// Design: a wave owns 32 token rows for the whole chain; nothing but the weights ever crosses waves.
//   * The wave loads its 32 x 320 rows once, normalises them in registers (row_stats / row_norm: a row lives in the two
//     lanes l, l + 32) and keeps them as the 20 B-operand fragments of v_mfma_f32_32x32x16_bf16 (80 VGPRs).
//   * The hidden dimension is walked in chunks of 32: [h_c ; g_c]^T = W1_c X^T (two D^T accumulator tiles, K = 320),
//     hid_c = h_c * gelu(g_c) stays in the accumulator layout -- column (token) on the lane, hidden index in the
//     registers -- which IS the B operand of the second product out^T += W2_c hid_c^T (guide: "an accumulator tile as the
//     next MFMA's operand"); its permuted k order is baked into the packed W2.  out^T (320 x 32 f32) = 160 accumulator
//     registers.  With 1 wave per SIMD the kernel has the whole 512-register file.
//   * Weights: one linear stream per layer, already in LDS image order (W1: slab_chunk / slab_off below), 60 KB per
//     iteration [W1 of chunk it | W2 of chunk it-2], copied by LDS-DMA into a 2-slot ring, one barrier per iteration
//     (the biases and the LayerNorm affine stay in LDS for the whole kernel).  Iteration `it` runs GEMM1(it), the GELU of
//     chunk it-1 and GEMM2(it-2): three independent register sets, so the GELU's VALU instructions and the ring's DMA
//     issues sit in the shadow of 60 MFMAs (<= 4 single-issue fillers per MFMA: MI355X_MICROARCH.md, "HIDDEN per gap").
//   * Epilogue: + b2 (accumulator init), D^T -> row-major through a wave-private LDS slab (slab_put), + residual, 16-byte
//     stores.
// rowlin_kernel, further down, is the same row-resident scheme for one Linear behind an optional LayerNorm: the same rows in
// registers, the same LayerNorm, weight-slab image and transpose slab.
// The h16 GELU here is x * sigmoid(x (a + b u + c u^2)), u = min(x^2, 64): |err| <= 2.6e-5 absolute against the erf form
// (h16 resolution at 1.0 is 3.9e-3); the fp32 parity mode never takes this path.
#include "common.h"

namespace dsim {
namespace {

constexpr int RC = 320;                       // channels
constexpr int RKS = RC / 16;                  // 20 k-steps of 16
constexpr int RNB = RC / 32;                  // 10 output column blocks of 32
constexpr int RNCH = 4 * RC / 32;             // 40 hidden chunks of 32
constexpr int RITER = RNCH + 2;               // 42 ring iterations per row tile (even: slot parity == iteration parity)
constexpr int RW1B = 64 * RC * 2;             // 40960: [h rows 32 | g rows 32] x K 320, five swizzled [64][128 B] slabs
constexpr int RW2B = RC * 64;                 // 20480: [320 rows][32 hidden], swizzled 16-B chunks
constexpr int RCHB = RW1B + RW2B;             // 61440 bytes per ring slot / stream chunk
constexpr int RPIECES = RCHB / 1024;          // 60 LDS-DMA pieces: 15 per wave, no tail
constexpr int RPW = RPIECES / 4;
// resident vectors (f32): b1 [8C] GEGLU-interleaved, b2 [C], LayerNorm gamma / beta [C]
constexpr int RB1 = 0, RB2 = 8 * RC, RLG = 9 * RC, RLB = 10 * RC, RVEC = 11 * RC;
constexpr int SLABP = 144;                    // row pitch of a wave's transpose slab: 64 columns of h16 + 16 bytes of padding
constexpr int RSCR = 32 * SLABP;              // per-wave transpose slab of the feed-forward: 32 rows
constexpr int RLDS = 2 * RCHB + RVEC * 4 + 4 * RSCR;     // 155392
static_assert(RPIECES % 4 == 0 && RITER % 2 == 0, "ring geometry");

// ---- the swizzled [rows][128 B] weight slab --------------------------------------------------------------------------------
// A block of weight rows x K = 320 (W1 of a hidden chunk: 64 rows; a rowlin block: 32 rows) lies in the stream, and so in the LDS
// ring, as five slabs of 64 k: [rows][128 B] each, the positions of row r's eight 16-byte chunks XORed with (r >> 1) & 7, so that
// the A-operand fragment reads -- 32 consecutive rows at one chunk -- do not all fall on the same banks.  slab_chunk() is the
// packers' side of it (which chunk of the row-major weight lies at chunk position cpos of slab row `row`), slab_off() the
// kernels' (the byte of a slab at which chunk c of row `row` is found).  They are inverses:
//     slab_off(row, slab_chunk(row, cpos)) == row * 128 + cpos * 16,
// because the XOR term is its own inverse; a change to one is a change to both.
__device__ __forceinline__ int slab_chunk(int row, int cpos) { return cpos ^ ((row >> 1) & 7); }
__device__ __forceinline__ int slab_off(int row, int c) { const int s = (row >> 1) & 7; return row * 128 + ((c ^ s) << 4); }
// The 16 bytes the image of weight rows [row0, row0 + rows) of the packed [N][320] matrix w holds at chunk position cpos of row
// `row` of slab `slab`.  (Byte o of an image is slab o / (rows * 128), row o % (rows * 128) / 128, position o % 128 / 16: the
// packers split o themselves -- split in here, hipcc narrows the arithmetic differently and their code changes.)
// ldw, k0: the row pitch of w and the first of the 320 k the image covers (a K = 640 rowlin block is two images: k0 = 0, 320).
__device__ __forceinline__ u32x4 slab_image(const h16* __restrict__ w, int row0, int slab, int row, int cpos, int ldw = RC, int k0 = 0) {
    const int cl = slab_chunk(row, cpos);
    return *reinterpret_cast<const u32x4*>(w + (size_t)(row0 + row) * ldw + k0 + 64 * slab + 8 * cl);
}

// stream chunk ci, 16-byte unit u: see the layout comment at the top (W1: the slab image of the chunk's 64 rows)
__global__ void pack_ff_stream_kernel(const h16* __restrict__ w1p, const h16* __restrict__ w2p, char* __restrict__ stream) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= RITER * (RCHB / 16)) return;
    const int ci = i / (RCHB / 16), o = (i - ci * (RCHB / 16)) * 16;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (o < RW1B) {
        if (ci < RNCH) v = slab_image(w1p, 64 * ci, o / 8192, (o % 8192) / 128, (o % 128) / 16);
    } else {
        if (ci >= 2) {
            const int c = ci - 2, o2 = o - RW1B;
            const int row = o2 / 64, cpos = (o2 % 64) / 16;
            const int cl = cpos ^ ((row >> 2) & 3);
            const int s = cl >> 1, hh = cl & 1;
            h16x8 e;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                e[j] = w2p[(size_t)row * (4 * RC) + 32 * c + 16 * s + 8 * (j >> 2) + 4 * hh + (j & 3)];
            v = __builtin_bit_cast(u32x4, e);
        }
    }
    *reinterpret_cast<u32x4*>(stream + (size_t)ci * RCHB + o) = v;
}

// ---- a wave's 32 rows in registers ------------------------------------------------------------------------------------------
// Row l31 of the tile lives in the lanes l31 and l31 + 32 as KS (RKS; 40 at 640 channels) raw h16 B-operand fragments: lane (l31, half) holds the columns
// 16 ks + 8 half .. + 7 in x[ks].  The LayerNorm is three passes over those registers (sum, centred squares, normalise): an f32
// copy of the rows would not fit beside them in the 256 architectural VGPRs the VALU can address.  row_stats() is the first two
// passes, row_norm() the third for one fragment; the kernels choose where the normalised fragment goes.
template <int KS>
__device__ __forceinline__ void row_stats(u32x4 (&x)[KS], float eps, float& mean, float& rstd) {
    float sum = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const h16x8 t = __builtin_bit_cast(h16x8, x[ks]);
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += (float)t[j];
    }
    sum = half_sum(sum);
    mean = sum * (1.0f / (16 * KS));
    float sq = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        asm volatile("" : "+v"(x[ks]));      // (opaque: keeps hipcc from carrying the f32 conversions from pass to pass)
        const h16x8 t = __builtin_bit_cast(h16x8, x[ks]);
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = (float)t[j] - mean; sq = fmaf(d, d, sq); }
    }
    sq = half_sum(sq);
    rstd = 1.0f / sqrtf(sq * (1.0f / (16 * KS)) + eps);
}
// gamma, beta: the resident f32 [16 KS] vectors in LDS
__device__ __forceinline__ h16x8 row_norm(u32x4& x, int ks, int half, float mean, float rstd, const float* gamma, const float* beta) {
    const int c = 16 * ks + 8 * half;
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + c), g1 = *reinterpret_cast<const f32x4*>(gamma + c + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + c), b1 = *reinterpret_cast<const f32x4*>(beta + c + 4);
    asm volatile("" : "+v"(x));
    const h16x8 t = __builtin_bit_cast(h16x8, x);
    h16x8 y;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        y[j] = (h16)fmaf(((float)t[j] - mean) * rstd, g0[j], b0[j]);
        y[4 + j] = (h16)fmaf(((float)t[4 + j] - mean) * rstd, g1[j], b1[j]);
    }
    return y;
}
// Epilogues: a 32 x 32 D^T accumulator tile (the lane's token on the lane, output column 8 q + 4 half + e in register 4 q + e)
// goes to row-major through a wave-private slab of SLABP-byte rows.  This is the lane's 16 values, as h16, into the slab row
// `srow` at the columns 32 bb .. 32 bb + 31.
__device__ __forceinline__ void slab_put(char* srow, int bb, int half, const f32x16& a) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        h16x4 pk;
#pragma unroll
        for (int e = 0; e < 4; ++e) pk[e] = (h16)a[4 * q + e];
        *reinterpret_cast<h16x4*>(srow + (bb * 32 + 8 * q + 4 * half) * 2) = pk;
    }
}

struct FFParams {
    const h16* x;          // [M][320] residual stream (input of the LayerNorm and the residual)
    h16* out;              // [M][320]; may alias x
    const float* ln_g;
    const float* ln_b;
    const char* stream;     // RITER * RCHB bytes
    const float* b1;        // [8C] GEGLU-interleaved
    const float* b2;
    int M;
    float eps;
    unsigned x_bytes, stream_bytes;
    int stagger;            // s_nop 7 units (8 wait states each) wave w idles after every ring barrier, times w
};

// DBG (development builds only, tools/kbench ablations; the product instantiates DBG = 0): 1 no weight DMA, 2 no GELU,
// 4 no GEMM1 MFMAs, 8 no GEMM2 MFMAs, 16 no fragment reads
template <int DBG>
__global__ __launch_bounds__(256, 1) void ff_fused_kernel(const FFParams p, const int ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    const __amdgpu_buffer_rsrc_t rX = buf_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t rO = buf_rsrc(p.out, p.x_bytes);
    const __amdgpu_buffer_rsrc_t rS = buf_rsrc(p.stream, p.stream_bytes);

    // ring: piece d (0..14) of this wave for stream chunk ci into the slot of parity sp; a wave copies 15 KB contiguous
    auto dma = [&](int sp, int ci, int d) {
        if (DBG & 1) return;
        char* dst = smem + sp * RCHB + wave * (RPW * 1024) + d * 1024;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rS, (__attribute__((address_space(3))) void*)dst, 16, lane * 16,
                                                 ci * RCHB + wave * (RPW * 1024) + d * 1024, 0, 0);
    };
#pragma unroll
    for (int d = 0; d < RPW; ++d) dma(0, 0, d);
    // the small vectors stay in LDS for the whole kernel
    float* const vec = reinterpret_cast<float*>(smem + 2 * RCHB);
    for (int i = tid; i < RVEC / 4; i += 256) {
        const int e = 4 * i;
        const float* src = e < RB2 ? p.b1 + e : (e < RLG ? p.b2 + (e - RB2) : (e < RLB ? p.ln_g + (e - RLG) : p.ln_b + (e - RLB)));
        *reinterpret_cast<f32x4*>(vec + e) = *reinterpret_cast<const f32x4*>(src);
    }

    // per-lane LDS read offsets inside a slot
    int w1off[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) w1off[kk] = slab_off(l31, 2 * kk + half);
    const int sw2 = (l31 >> 2) & 3;
    int w2off[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) w2off[s] = RW1B + l31 * 64 + (((2 * s + half) ^ sw2) << 4);

    // rows of a tile as raw h16 B-operand fragments: lane (l31, half) holds columns 16 ks + 8 half .. + 7 of row l31
    u32x4 raw[RKS];
    auto load_rows = [&](int tile) {
        const int row = tile * 128 + wave * 32 + l31;
        const unsigned rbase = (tile < ntiles && row < p.M) ? (unsigned)row * (RC * 2) + half * 16 : BUF_OOB;
#pragma unroll
        for (int ks = 0; ks < RKS; ++ks) raw[ks] = __builtin_amdgcn_raw_buffer_load_b128(rX, (int)(rbase + ks * 32), 0, 0);
    };
    load_rows(blockIdx.x);
    __syncthreads();      // the resident vectors are in LDS

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int m0 = tile * 128 + wave * 32;
        // ---- LayerNorm in registers -> B-operand fragments ---------------------------------------
        h16x8 X[RKS];
        {
            float mean, rstd;
            row_stats(raw, p.eps, mean, rstd);
#pragma unroll
            for (int ks = 0; ks < RKS; ++ks) X[ks] = row_norm(raw[ks], ks, half, mean, rstd, vec + RLG, vec + RLB);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- out^T accumulators start at b2 ----------------------------------------------------
        f32x16 out[RNB];
#pragma unroll
        for (int b = 0; b < RNB; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 b4 = *reinterpret_cast<const f32x4*>(vec + RB2 + 32 * b + 8 * q + 4 * half);
#pragma unroll
                for (int e = 0; e < 4; ++e) out[b][4 * q + e] = b4[e];
            }
        __builtin_amdgcn_sched_barrier(0);

        f32x16 aH[2], aG[2];      // GEMM1 accumulator sets (chunk parity)
        h16x8 wf[2][4];          // double-buffered weight fragments: group n reads set n & 1 while set (n + 1) & 1 loads
        h16x8 p0, p1;            // h * gelu(g) of chunk it-2: the two k-steps of GEMM2's B operand
        h16x8 q0, q1;            // ... of chunk it-1, being produced
        float hv[16];

        // wave w idles w * stagger units after each ring barrier: the loop lives inside one asm statement, so hipcc's
        // control-flow graph (and with it the pinned schedule and the register allocation) does not see a branch here
        auto stagger_wait = [&]() {
            int cnt = wave * p.stagger;
            asm volatile("s_cmp_eq_u32 %0, 0\n\ts_cbranch_scc1 .Lstag_end_%=\n.Lstag_%=:\n\ts_nop 7\n\ts_sub_u32 %0, %0, 1\n\t"
                         "s_cmp_lg_u32 %0, 0\n\ts_cbranch_scc1 .Lstag_%=\n.Lstag_end_%=:" : "+s"(cnt) :: "scc");
        };
        // accumulators of chunk c start at its b1 slice
        auto init1 = [&](int c, f32x16& h, f32x16& gg) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 bh = *reinterpret_cast<const f32x4*>(vec + RB1 + 64 * c + 8 * q + 4 * half);
                const f32x4 bg = *reinterpret_cast<const f32x4*>(vec + RB1 + 64 * c + 32 + 8 * q + 4 * half);
#pragma unroll
                for (int e = 0; e < 4; ++e) { h[4 * q + e] = bh[e]; gg[4 * q + e] = bg[e]; }
            }
        };
        // GEMM1 group i = k-steps 2i, 2i+1: fragments [h(2i), g(2i), h(2i+1), g(2i+1)]
        auto ld1 = [&](const char* slot, int i, h16x8 (&w)[4]) {
            if ((DBG & 16) && i > 0) return;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int ks = 2 * i + u;
                const char* a = slot + (ks >> 2) * 8192 + w1off[ks & 3];
                w[2 * u] = *reinterpret_cast<const h16x8*>(a);
                w[2 * u + 1] = *reinterpret_cast<const h16x8*>(a + 32 * 128);
            }
        };
        auto mm1 = [&](int i, const h16x8 (&w)[4], f32x16& h, f32x16& gg) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (DBG & 4) { asm volatile("" :: "v"(w[2 * u]), "v"(w[2 * u + 1]), "v"(X[2 * i + u])); continue; }
                h = H16_MFMA_32x32x16(w[2 * u], X[2 * i + u], h, 0, 0, 0);
                gg = H16_MFMA_32x32x16(w[2 * u + 1], X[2 * i + u], gg, 0, 0, 0);
            }
        };
        // GEMM2 group j = output blocks 2j, 2j+1: fragments [b(2j) s0, b(2j) s1, b(2j+1) s0, b(2j+1) s1]
        auto ld2 = [&](const char* slot, int j, h16x8 (&w)[4]) {
            if (DBG & 16) return;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                w[2 * u] = *reinterpret_cast<const h16x8*>(slot + w2off[0] + (2 * j + u) * 2048);
                w[2 * u + 1] = *reinterpret_cast<const h16x8*>(slot + w2off[1] + (2 * j + u) * 2048);
            }
        };
        auto mm2 = [&](int j, const h16x8 (&w)[4]) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (DBG & 8) { asm volatile("" :: "v"(w[2 * u]), "v"(w[2 * u + 1]), "v"(p0), "v"(p1)); continue; }
                out[2 * j + u] = H16_MFMA_32x32x16(w[2 * u], p0, out[2 * j + u], 0, 0, 0);
                out[2 * j + u] = H16_MFMA_32x32x16(w[2 * u + 1], p1, out[2 * j + u], 0, 0, 0);
            }
        };
        // element e of h * gelu(g) of the previous chunk; pairs are packed as soon as the odd one exists
        auto geglu1 = [&](int e, const f32x16& h, const f32x16& gg) {
            hv[e] = (DBG & 2) ? h[e] + gg[e] : h[e] * gelu_fast(gg[e]);
            if (e & 1) {
                if (e < 8) { q0[e - 1] = (h16)hv[e - 1]; q0[e] = (h16)hv[e]; }
                else { q1[e - 9] = (h16)hv[e - 1]; q1[e - 8] = (h16)hv[e]; }
            }
        };
        // One iteration, pinned group by group (left alone hipcc issues every ds_read right before its MFMA, and a lone wave
        // per SIMD then waits out the LDS latency 60 times per iteration): the fragments of group n+1 are requested, then
        // group n's four MFMAs issue with their share of the GELU and of the ring's DMA pieces between them.  Groups 0-9:
        // GEMM1(c); groups 10-14: GEMM2(c-2); the 16 GELU elements of chunk c-1 and the 15 DMA pieces of the next iteration
        // (those in the first half of the groups, so that they have landed by the next barrier) are dealt over the groups.
        // PAR = parity of the iteration (ring slot and GEMM1 accumulator set), a literal; C = chunk index (may be a variable).
#define RR_SB __builtin_amdgcn_sched_barrier(0)
#define RR_MIX(NV)                                                                                                    \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);         \
        __builtin_amdgcn_sched_group_barrier(0x002, NV, 0);                                                           \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);         \
        __builtin_amdgcn_sched_group_barrier(0x002, NV, 0);                                                           \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, NV, 0);        \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, NV, 0);
#define RR_BODY(PAR, C, G1, GL, G2, NEXT_CI)                                                                          \
        {                                                                                                             \
            constexpr int NG = ((G1) ? 10 : 0) + ((G2) ? 5 : 0), NH = NG == 15 ? 12 : (NG == 10 ? 8 : 4);             \
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                          \
            __syncthreads();                                                                                          \
            stagger_wait();                        /* de-phase the four waves */                                      \
            const char* slot = smem + (PAR) * RCHB;                                                                   \
            if (G1) { init1((C), aH[PAR], aG[PAR]); ld1(slot, 0, wf[0]); } else ld2(slot, 0, wf[0]);                  \
            RR_SB;                                                                                                    \
            _Pragma("unroll") for (int n = 0; n < NG; ++n) {                                                          \
                const int gi = (G1) ? n : n + 10;          /* group id: 0-9 GEMM1, 10-14 GEMM2 */                     \
                if (n + 1 < NG) { if (gi + 1 < 10) ld1(slot, gi + 1, wf[(n + 1) & 1]); else ld2(slot, gi + 1 - 10, wf[(n + 1) & 1]); } \
                RR_SB;                                                                                                \
                if (gi < 10) mm1(gi, wf[n & 1], aH[PAR], aG[PAR]); else mm2(gi - 10, wf[n & 1]);                      \
                _Pragma("unroll") for (int d = 0; d < RPW; ++d) if ((d * NH) / RPW == n) dma((PAR) ^ 1, (NEXT_CI), d); \
                if (GL) { _Pragma("unroll") for (int e = 0; e < 16; ++e) if ((e * NG) / 16 == n) geglu1(e, aH[(PAR) ^ 1], aG[(PAR) ^ 1]); } \
                RR_MIX(4)                                                                                             \
                RR_SB;                                                                                                \
            }                                                                                                         \
            if (GL) { p0 = q0; p1 = q1; }                                                                             \
        }
        RR_BODY(0, 0, true, false, false, 1)
        RR_BODY(1, 1, true, true, false, 2)
        for (int c = 2; c < RNCH; c += 2) {          // two iterations per trip: every register-set index stays static
            RR_BODY(0, c, true, true, true, c + 1)
            RR_BODY(1, c + 1, true, true, true, c + 2)
        }
        // X is dead from here: request the next tile's rows under the two drain iterations
        load_rows(tile + (int)gridDim.x);
        RR_BODY(0, RNCH, false, true, true, RNCH + 1)
        RR_BODY(1, RNCH + 1, false, false, true, 0)
#undef RR_BODY
#undef RR_MIX
#undef RR_SB

        // ---- epilogue: D^T -> row-major through the wave's LDS slab, + residual, 16-byte stores ----
        char* const slab = smem + 2 * RCHB + RVEC * 4 + wave * RSCR;
        // read-back geometry: per pass (64 columns) 32 rows x 8 chunks of 16 B = 256 pieces, 4 per lane
        u32x4 res[RNB / 2][4];
#pragma unroll
        for (int pp = 0; pp < RNB / 2; ++pp)
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int idx = lane + it * 64, r = idx >> 3, c = idx & 7;
                const unsigned go = (m0 + r) < p.M ? (unsigned)(m0 + r) * (RC * 2) + (unsigned)(pp * 128 + c * 16) : BUF_OOB;
                res[pp][it] = __builtin_amdgcn_raw_buffer_load_b128(rX, (int)go, 0, 0);
            }
#pragma unroll
        for (int pp = 0; pp < RNB / 2; ++pp) {
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) slab_put(slab + l31 * SLABP, bb, half, out[2 * pp + bb]);
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int idx = lane + it * 64, r = idx >> 3, c = idx & 7;
                const unsigned go = (m0 + r) < p.M ? (unsigned)(m0 + r) * (RC * 2) + (unsigned)(pp * 128 + c * 16) : BUF_OOB;
                const h16x8 t = *reinterpret_cast<const h16x8*>(slab + r * SLABP + c * 16);
                const h16x8 rr = __builtin_bit_cast(h16x8, res[pp][it]);
                h16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (h16)((float)t[e] + (float)rr[e]);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rO, (int)go, 0, 0);
            }
        }
    }
    // the last DMA pieces of this workgroup (the next tile's chunk 0) are still in flight: drain before exit
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- row-resident Linear (optionally behind a LayerNorm or a GroupNorm's per-image affine) for K = 320 and K = 640 -----------
// out[M][N] = P(x)[M][K] W^T (+ bias), N a multiple of 64: the fused to_q/to_k/to_v projection behind norm1 (N = 3 K) and
// attn2.to_q behind norm2 (hacked_modules.py:88-116), and proj_in behind the Transformer2DModel's GroupNorm.  The tiled GEMM is
// latency-bound on these: a K of five tiles leaves its two-stage ring one 1.2 us K step of cover for activations that stream from
// HBM exactly once (726 TF/s, 3.0 TB/s at N = 960), and the normalisation in front costs a full read + write of the tensor.  Here a
// wave keeps its 32 rows in registers (normalised on arrival), the weights stream through a 2-slot LDS ring in 32-column blocks,
// the output leaves in 128-byte row segments per pair of blocks -- HBM-bound, one pass.
// One body (rowlin_body) behind thin kernels:
//   rowlin_kernel<DBG>         K = 320, LayerNorm where p.ln_g.  Three 4-wave workgroups per CU (__launch_bounds__(256, 3): <= 168
//                              registers; 52736 bytes of LDS each): one workgroup's row loads and stores sit under the others' MFMAs.
//   rowlin640_kernel<DBG>      K = 640, the same.  A wave's rows are 40 fragments (160 registers): two workgroups per CU.  The ring
//                              slot stays 32 columns x 320 k; a column block takes two ring steps into the same accumulator.
//   gn_rowlin_kernel<K, DBG>   the GroupNorm form: where p.coef, y = (h16) fmaf(x, sc[b][c], sh[b][c]) on arrival -- gn_apply_kernel's
//                              expression and rounding point (norm.hip), so the rows that enter the MFMAs are the bits the unfused
//                              GroupNorm writes -- and an f32 bias as the accumulators' initial value.  The coefficients come from
//                              a table [B][2][K] f32 that the statistics pass leaves (launch_groupnorm_stats), not from a fold of
//                              the image's partials in every tile: the table is 2 K floats per tile from L2 against up to 16 KB of
//                              f64 partials.  A 128-row tile lies inside one image (HW % 128 == 0).
constexpr int LCHB = 32 * RC * 2;              // 20480 bytes per ring slot: W rows [32 b, 32 b + 32) x 320 k, five [32][128 B] slabs
constexpr int LPW = LCHB / 1024 / 4;           // 5 DMA pieces per wave per ring step
constexpr int LSCR = 16 * SLABP;               // per-wave transpose slab: 16 rows
// resident f32: [gamma K | beta K] (LayerNorm) or the tile's image's [sc K | sh K]; the GroupNorm form's bias [K] (N <= K there)
constexpr int rowlin_lds(int K, bool GN) { return 2 * LCHB + 2 * K * 4 + (GN ? K * 4 : 0) + 4 * LSCR; }
static_assert(rowlin_lds(RC, false) == 52736, "three workgroups per CU");

// stream = the ring steps in order: column block b, then (K = 640) its k half
__global__ void pack_rowlin_stream_kernel(const h16* __restrict__ wp, char* __restrict__ stream, int N, int K) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int kh = K / RC;
    if (i >= N / 32 * kh * (LCHB / 16)) return;
    const int t = i / (LCHB / 16), o = (i - t * (LCHB / 16)) * 16;
    *reinterpret_cast<u32x4*>(stream + (size_t)t * LCHB + o) =
        slab_image(wp, 32 * (t / kh), o / 4096, (o % 4096) / 128, (o % 128) / 16, K, RC * (t % kh));
}

struct RLParams {
    const h16* x;
    h16* out;
    const float* ln_g;      // null: no LayerNorm
    const float* ln_b;
    const char* stream;
    int M, N;
    float eps;
    unsigned x_bytes, out_bytes, stream_bytes;
    // the GroupNorm form only
    const float* coef;      // [B][2][K] f32: sc, sh of every image; null: no prologue
    const float* bias;      // [N] f32 or null
    int HW;                 // rows per image
};

// DBG: kbench ablation masks (1 no output stores, 2 no MFMAs, 4 no row loads, 8 no fragment reads); 0 in the product
template <int K, bool GN, int DBG>
__device__ __forceinline__ void rowlin_body(const RLParams& p, const int ntiles) {
    constexpr int KS = K / 16, KH = K / RC;     // fragments of a row; ring steps per column block
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const __amdgpu_buffer_rsrc_t rX = buf_rsrc(p.x, p.x_bytes);
    const __amdgpu_buffer_rsrc_t rO = buf_rsrc(p.out, p.out_bytes);
    const __amdgpu_buffer_rsrc_t rS = buf_rsrc(p.stream, p.stream_bytes);
    const int nblk = p.N / 32 * KH;            // ring steps per tile; even
    auto dma = [&](int sp, int blk) {           // this wave's five pieces of ring step `blk` into the slot of parity sp
        char* dst = smem + sp * LCHB + wave * (LPW * 1024);
#pragma unroll
        for (int d = 0; d < LPW; ++d)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rS, (__attribute__((address_space(3))) void*)(dst + d * 1024), 16, lane * 16,
                                                     blk * LCHB + wave * (LPW * 1024) + d * 1024, 0, 0);
    };
    dma(0, 0);
    float* const vec = reinterpret_cast<float*>(smem + 2 * LCHB);         // [gamma K | beta K], or [sc K | sh K] of the tile's image
    float* const bvec = vec + 2 * K;                                      // GN: bias [K], zeros past N and without one
    if (GN) {
        for (int i = tid; i < K; i += 256) bvec[i] = (p.bias && i < p.N) ? p.bias[i] : 0.f;
    } else if (p.ln_g) {
        for (int i = tid; i < 2 * K; i += 256) vec[i] = i < K ? p.ln_g[i] : p.ln_b[i - K];
    }
    char* const slab = smem + rowlin_lds(K, GN) - 4 * LSCR + wave * LSCR;
    int woff[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) woff[kk] = slab_off(l31, 2 * kk + half);
    __syncthreads();
    int blk = 0;                                // the ring step the NEXT one consumes (wraps at nblk: same weights for every tile)

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int m0 = tile * 128 + wave * 32;
        // the rows live in ONE register array: raw h16 on arrival, overwritten in place by their normalised values
        u32x4 xr[KS];
        {
            const int row = m0 + l31;
            const unsigned rbase = row < p.M ? (unsigned)row * (K * 2) + half * 16 : BUF_OOB;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                xr[ks] = (DBG & 4) ? u32x4{(unsigned)ks, 1u, 2u, rbase} : __builtin_amdgcn_raw_buffer_load_b128(rX, (int)(rbase + ks * 32), 0, 0);
            if (GN) {
                if (p.coef) {
                    // the image's coefficients into LDS.  Every wave has left the previous tile's prologue: it passed that tile's
                    // ring barriers since.
                    const float* src = p.coef + (size_t)(tile * 128 / p.HW) * (2 * K);
                    for (int i = tid; i < 2 * K / 4; i += 256)
                        *reinterpret_cast<f32x4*>(vec + 4 * i) = *reinterpret_cast<const f32x4*>(src + 4 * i);
                    __syncthreads();
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        const int c = 16 * ks + 8 * half;
                        const f32x4 s0 = *reinterpret_cast<const f32x4*>(vec + c), s1 = *reinterpret_cast<const f32x4*>(vec + c + 4);
                        const f32x4 h0 = *reinterpret_cast<const f32x4*>(vec + K + c), h1 = *reinterpret_cast<const f32x4*>(vec + K + c + 4);
                        const h16x8 t = __builtin_bit_cast(h16x8, xr[ks]);
                        h16x8 y;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            // two roundings, f32 then h16, as gn_apply_kernel's: left to itself hipcc fuses the pair into one
                            // v_fma_mixlo_f16, which rounds once -- other bits in about one fp16 value of 10^4
                            float f0 = fmaf((float)t[j], s0[j], h0[j]), f1 = fmaf((float)t[4 + j], s1[j], h1[j]);
                            asm("" : "+v"(f0), "+v"(f1));
                            y[j] = (h16)f0;
                            y[4 + j] = (h16)f1;
                        }
                        xr[ks] = __builtin_bit_cast(u32x4, y);
                    }
                }
            } else if (p.ln_g) {                // in place, fragment by fragment
                float mean, rstd;
                row_stats(xr, p.eps, mean, rstd);
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    xr[ks] = __builtin_bit_cast(u32x4, row_norm(xr[ks], ks, half, mean, rstd, vec, vec + K));
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // one ring step: 20 MFMAs of 32 output columns x 320 k (k half `kh` of the rows) into `a`, fragments double-buffered by
        // 64-wide K slab.  kh == 0 starts the accumulator (GN: at the bias of the columns from `col`).
        h16x8 wf[2][2];
        auto step = [&](int sp, f32x16& a, int kh, bool stored, int col) {
            // the slot's five DMA pieces must have landed; the four row-segment stores of the previous pair were issued after the
            // pieces of the step before a `stored` one (vmcnt retires in issue order on gfx9): leave them in flight there
            if (stored) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            const int nb = blk + 1 == nblk ? 0 : blk + 1;
            dma(sp ^ 1, nb);
            blk = nb;
            const char* slot = smem + sp * LCHB;
            if (kh == 0) {
                if (GN) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 b4 = *reinterpret_cast<const f32x4*>(bvec + col + 8 * q + 4 * half);
#pragma unroll
                        for (int e = 0; e < 4; ++e) a[4 * q + e] = b4[e];
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 16; ++e) a[e] = 0.f;
                }
            }
            auto ld = [&](int i, h16x8 (&w)[2]) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int ks = 2 * i + u;
                    w[u] = *reinterpret_cast<const h16x8*>(slot + (ks >> 2) * 4096 + woff[ks & 3]);
                }
            };
            ld(0, wf[0]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 10; ++i) {
                if (i < 9 && !(DBG & 8)) ld(i + 1, wf[(i + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (!(DBG & 2)) a = H16_MFMA_32x32x16(wf[i & 1][u], __builtin_bit_cast(h16x8, xr[RKS * kh + 2 * i + u]), a, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        // a pair of blocks = 64 output columns = 128-byte row segments: D^T -> row-major through the wave's 16-row slab in two
        // passes (rows 0-15, 16-31), 16-byte stores of full lines
        auto store_pair = [&](const f32x16& a0, const f32x16& a1, int col0) {
#pragma unroll
            for (int ph = 0; ph < 2; ++ph) {
                asm volatile("" ::: "memory");       // pass 1 overwrites the slab pass 0 is read from
                if ((l31 >> 4) == ph) {      // (a loop over the pair: as two calls, hipcc assigns this kernel's registers differently)
#pragma unroll
                    for (int bb = 0; bb < 2; ++bb) slab_put(slab + (l31 & 15) * SLABP, bb, half, bb ? a1 : a0);
                }
#pragma unroll
                for (int it = 0; it < 2; ++it) {
                    const int idx = lane + it * 64, r = idx >> 3, c = idx & 7, row = m0 + 16 * ph + r;
                    const unsigned go = row < p.M ? ((unsigned)row * (unsigned)p.N + (unsigned)col0) * 2u + (unsigned)c * 16u : BUF_OOB;
                    const u32x4 t = *reinterpret_cast<const u32x4*>(slab + r * SLABP + c * 16);
                    if (!(DBG & 1) || t[0] == 0x12345u) __builtin_amdgcn_raw_buffer_store_b128(t, rO, (int)go, 0, 0);
                }
            }
        };
        f32x16 a0, a1;
        for (int pr = 0; pr < p.N / 64; ++pr) {
            if (KH == 1) {
                step(0, a0, 0, true, 64 * pr);
                step(1, a1, 0, false, 64 * pr + 32);
            } else {
                step(0, a0, 0, true, 64 * pr);
                step(1, a0, 1, false, 64 * pr);
                step(0, a1, 0, false, 64 * pr + 32);
                step(1, a1, 1, false, 64 * pr + 32);
            }
            store_pair(a0, a1, 64 * pr);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int DBG>
__global__ __launch_bounds__(256, 3) void rowlin_kernel(const RLParams p, const int ntiles) { rowlin_body<RC, false, DBG>(p, ntiles); }
template <int DBG>
__global__ __launch_bounds__(256, 2) void rowlin640_kernel(const RLParams p, const int ntiles) { rowlin_body<2 * RC, false, DBG>(p, ntiles); }
template <int K, int DBG>
__global__ __launch_bounds__(256, K == RC ? 3 : 2) void gn_rowlin_kernel(const RLParams p, const int ntiles) { rowlin_body<K, true, DBG>(p, ntiles); }

// The launch of either row-resident kernel: 128-row tiles, dealt to a persistent grid of at most wpc workgroups per CU
template <auto Kern, typename P>
int launch_rows(const P& p, int wpc, int lds, hipStream_t s) {
    const int ntiles = (p.M + 127) / 128, cap = wpc * cu_count();
    return launch_lds<Kern>(dim3(ntiles < cap ? ntiles : cap), dim3(256), lds, s, p, ntiles);
}

}  // namespace

#ifdef DSIM_DEVTOOLS
int g_rl_dbg = 0;
int g_ff_dbg = 0;
int g_ff_stagger = -1;     // -1 = the product default
int g_rl_wpc = 3;          // rowlin_kernel's persistent workgroups per CU
#endif

inline namespace DSIM_H16_NS {
size_t ff_stream_bytes(int C) { return C == RC ? (size_t)RITER * RCHB : 0; }

int pack_ff_stream(const void* w1_packed, const void* w2_packed, void* stream, int C, hipStream_t s) {
    if (C != RC) return DSIM_ERR_INVALID;
    const int n = RITER * (RCHB / 16);
    hipLaunchKernelGGL(pack_ff_stream_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const h16*)w1_packed,
                       (const h16*)w2_packed, (char*)stream);
    DSIM_HIP_CHECK(hipGetLastError());
    return DSIM_OK;
}

int launch_ff_fused(const FFArgs& a, hipStream_t s) {
    if (a.dtype != DSIM_H16) return a.dtype == DSIM_F16 ? DSIM_F16_TWIN(launch_ff_fused(a, s)) : DSIM_ERR_INVALID;
    if (a.C != RC || a.M < 1 || (size_t)a.M * RC * 2 >= 0x7fffffffull) return DSIM_ERR_INVALID;
    FFParams p;
    p.x = (const h16*)a.x; p.out = (h16*)a.out; p.ln_g = a.ln_g; p.ln_b = a.ln_b; p.stream = (const char*)a.stream;
    p.b1 = a.b1; p.b2 = a.b2; p.M = a.M; p.eps = a.eps;
    p.x_bytes = (unsigned)((size_t)a.M * RC * 2);
    p.stream_bytes = (unsigned)((size_t)RITER * RCHB);
    // The four waves of a workgroup leave every ring barrier together and issue their DMA pieces and fragment reads at the same
    // instants; de-phased by one 8-wait-state unit per wave index the kernel runs 1.7 % faster (interleaved-round sweep in
    // profiles/r03_ff_fused_ablation.txt: 0 -> 1.208, 1 -> 1.187, 2 -> 1.218, 3 -> 1.246 ms).
    p.stagger = g_ff_stagger >= 0 ? g_ff_stagger : 1;
#ifdef DSIM_DEVTOOLS
    switch (g_ff_dbg) {             // tools/kbench: the ablation variant, if it is one of those compiled in
#define X(d) case d: return launch_rows<ff_fused_kernel<d>>(p, 1, RLDS, s);
        X(1) X(2) X(3) X(12) X(13) X(15) X(16) X(31)
#undef X
        default: break;
    }
#endif
    return launch_rows<ff_fused_kernel<0>>(p, 1, RLDS, s);
}

size_t rowlin_stream_bytes(int C, int N) {
    return ((C == RC || C == 2 * RC) && N >= 64 && N % 64 == 0 && N <= 3 * C) ? (size_t)N / 32 * (C / RC) * LCHB : 0;      // up to q|k|v
}

int pack_rowlin_stream(const void* w_packed, void* stream, int C, int N, hipStream_t s) {
    if (!rowlin_stream_bytes(C, N)) return DSIM_ERR_INVALID;
    const int n = N / 32 * (C / RC) * (LCHB / 16);
    hipLaunchKernelGGL(pack_rowlin_stream_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const h16*)w_packed, (char*)stream, N, C);
    DSIM_HIP_CHECK(hipGetLastError());
    return DSIM_OK;
}

int launch_rowlin(const RowLinArgs& a, hipStream_t s) {
    if (a.dtype != DSIM_H16) return a.dtype == DSIM_F16 ? DSIM_F16_TWIN(launch_rowlin(a, s)) : DSIM_ERR_INVALID;
    if (!rowlin_stream_bytes(a.C, a.N) || a.M < 1 || (size_t)a.M * a.N * 2 >= 0x7fffffffull || (size_t)a.M * a.C * 2 >= 0x7fffffffull ||
        !a.ln_g != !a.ln_b) return DSIM_ERR_INVALID;
    // the GroupNorm form: no LayerNorm beside it, N <= K (its bias lives in K floats of LDS), whole 128-row tiles per image
    if (a.gn && (a.ln_g || a.N > a.C || (a.coef && (a.HW < 128 || a.HW % 128 || a.M % a.HW)))) return DSIM_ERR_INVALID;
    if (!a.gn && (a.coef || a.bias)) return DSIM_ERR_INVALID;
    RLParams p;
    p.x = (const h16*)a.x; p.out = (h16*)a.out; p.ln_g = a.ln_g; p.ln_b = a.ln_b; p.stream = (const char*)a.stream;
    p.M = a.M; p.N = a.N; p.eps = a.eps;
    p.x_bytes = (unsigned)((size_t)a.M * a.C * 2); p.out_bytes = (unsigned)((size_t)a.M * a.N * 2);
    p.stream_bytes = (unsigned)rowlin_stream_bytes(a.C, a.N);
    p.coef = a.coef; p.bias = a.bias; p.HW = a.HW > 0 ? a.HW : 1;
    if (a.gn)
        return a.C == RC ? launch_rows<gn_rowlin_kernel<RC, 0>>(p, 3, rowlin_lds(RC, true), s)
                         : launch_rows<gn_rowlin_kernel<2 * RC, 0>>(p, 2, rowlin_lds(2 * RC, true), s);
    if (a.C != RC) return launch_rows<rowlin640_kernel<0>>(p, 2, rowlin_lds(2 * RC, false), s);
#ifdef DSIM_DEVTOOLS
    switch (g_rl_dbg) {
#define X(d) case d: return launch_rows<rowlin_kernel<d>>(p, g_rl_wpc, rowlin_lds(RC, false), s);
        X(1) X(2) X(4) X(8) X(10) X(15)
#undef X
        default: break;
    }
#endif
    return launch_rows<rowlin_kernel<0>>(p, g_rl_wpc, rowlin_lds(RC, false), s);
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
