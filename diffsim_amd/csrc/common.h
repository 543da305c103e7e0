// Internal shared declarations for libdiffsim_amd (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/diffsim_amd.h"

namespace dsim {

// The 16-bit compute type.  The kernel sources gemm / gemm_skinny / rowres / attention / tails / attn160 .hip are written against ONE
// 16-bit type, h16, and are compiled twice (diffsim_amd/build.py): once with h16 = bf16 (compute dtype DSIM_BF16, the headline
// mode) and once with -DDSIM_H16_IS_F16, h16 = IEEE fp16 (DSIM_F16: the arithmetic type the reference's drivers run in,
// /root/reference/cute_main.py:31, diffsim/diffsim.py:82).  Their host entry points (h16_api.h) live in the inline namespace
// DSIM_H16_NS, dsim::bf16 or dsim::f16: every caller names them unqualified and reaches the functions of its own compilation, and
// the bf16 ones forward DSIM_F16 calls with DSIM_F16_TWIN (below).  The kernels stay in dsim::(anonymous namespace).
// v_mfma_f32_16x16x32_f16 / v_mfma_f32_32x32x16_f16 take the same cycles as the bf16 forms, so tiles and schedules are shared.
typedef __bf16 bf16_t;
typedef _Float16 f16_t;
#ifdef DSIM_H16_IS_F16
typedef _Float16 h16;
#define DSIM_H16_NS f16
#define DSIM_H16 DSIM_F16
#define DSIM_H16_ONE_BITS 0x3C00u
// fixed-reference softmax (attn_core.h attend<FAST>): P = exp2(s - m0) is stored in the 16-bit type; fp16 tops out at 65504, so
// a row whose sum reaches 3e4 (a single P near the limit, or thousands of keys a few units above tile 0's maximum) takes the exact
// running-maximum form instead (in bf16 the bound is the f32 exponent range)
#define DSIM_H16_LSUM_MAX 3.0e4f
#define H16_MFMA_16x16x32 __builtin_amdgcn_mfma_f32_16x16x32_f16
#define H16_MFMA_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_f16
#else
typedef __bf16 h16;
#define DSIM_H16_NS bf16
#define DSIM_H16 DSIM_BF16
#define DSIM_H16_ONE_BITS 0x3F80u
#define DSIM_H16_LSUM_MAX 1e30f
#define H16_MFMA_16x16x32 __builtin_amdgcn_mfma_f32_16x16x32_bf16
#define H16_MFMA_32x32x16 __builtin_amdgcn_mfma_f32_32x32x16_bf16
#endif
typedef __attribute__((ext_vector_type(8))) h16 h16x8;
typedef __attribute__((ext_vector_type(4))) h16 h16x4;
typedef __attribute__((ext_vector_type(2))) h16 h16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

#ifdef __HIPCC__
// ds_read_b64_tr_b16 of the 16-bit compute type: p is a (generic) pointer into LDS
__device__ __forceinline__ h16x4 h16_ds_read_tr16_b64(const char* p) {
#ifdef DSIM_H16_IS_F16
    typedef __fp16 fp16v4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
    return __builtin_bit_cast(h16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16v4*)(p)));
#else
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) h16x4*)(p));
#endif
}
// GELU (erf form, F.gelu's default) for h16 outputs: x * sigmoid(x (a + b u + c u^2)), u = min(x^2, 64), with -log2(e) folded
// into the constants (the clamp keeps the odd quintic monotone).  |error| <= 2.6e-5 absolute, <= 0.3 h16 ulp of the result:
// one v_exp, one v_rcp and 7 plain VALU operations against 16 + 2 for the erf polynomial the fp32 parity mode keeps.  Used by
// every h16 GEGLU (the GEMM epilogue and the fused feed-forward), so the fused and unfused chains round alike.
__device__ __forceinline__ float gelu_fast(float x) {
    const float u = fminf(x * x, 64.0f);
    const float t = x * fmaf(u, fmaf(u, 1.01426306e-3f, -0.106775724f), -2.30112134f);
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t));
}
// The two 32-lane halves of a wave combined in every lane: one v_permlane32_swap (gfx950) instead of a ds_bpermute round trip
// through the LDS pipe.  A row of a 32 x 32 MFMA tile lives in the lanes l and l + 32, so these finish a per-row reduction: the
// softmax maximum (branched on once per key tile), a softmax denominator, a LayerNorm sum.
__device__ __forceinline__ float max_halves(float x) {
    const unsigned u = __float_as_uint(x);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);     // r[0] = lower half, r[1] = upper half, in both
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float half_sum(float x) {
    const unsigned u = __float_as_uint(x);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// Raw buffer descriptor over [ptr, ptr + bytes) for the __builtin_amdgcn_raw_buffer_* accesses (the last word: 32-bit data format,
// no stride or swizzle).  An access whose offset reaches `bytes` reads zeros and stores nothing; BUF_OOB is the voffset that is
// past the end of every buffer, the one a lane without an element passes.  (__attribute__((const)): a descriptor an instantiation
// never uses is then dropped before inlining, as the bare builtin was; without it the gemm_kernel instantiations that rebuild
// their output descriptor per tile come out with other register assignments.)
constexpr unsigned BUF_OOB = 0x80000000u;
__device__ __forceinline__ __attribute__((const)) __amdgpu_buffer_rsrc_t buf_rsrc(const void* ptr, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)ptr, 0, (int)bytes, 0x00020000);
}
#endif

#define DSIM_HIP_CHECK(expr)                                   \
    do {                                                       \
        hipError_t _e = (expr);                                \
        if (_e != hipSuccess) return DSIM_ERR_HIP;             \
    } while (0)

static inline size_t dtype_size(int dt) { return dt == DSIM_F32 ? 4 : 2; }
static inline const char* dtype_name(int dt) { return dt == DSIM_F32 ? "f32" : (dt == DSIM_F16 ? "f16" : "bf16"); }

// f(Elem<T>{}) for the element type T of `dtype`: the one switch from a run-time compute dtype to the kernels' template parameter
// (inside f: typename decltype(e)::type).  DSIM_ERR_INVALID for anything else.
template <typename T> struct Elem { typedef T type; };
template <typename F>
int by_dtype(int dtype, F&& f) {
    switch (dtype) {
        case DSIM_BF16: return f(Elem<bf16_t>{});
        case DSIM_F16: return f(Elem<f16_t>{});
        case DSIM_F32: return f(Elem<float>{});
    }
    return DSIM_ERR_INVALID;
}
// The same switch in a source compiled once per 16-bit type (h16_api.h), to the types this object's kernels are instantiated for:
// f(Elem<h16>{}) for the object's own 16-bit dtype in every object and f(Elem<float>{}) for DSIM_F32 in the bf16 objects alone -- the
// fp16 objects instantiate no f32 kernel.  DSIM_F16 seen from a bf16 object is its twin's: twin() forwards the call, written at the
// call site as [&] { return DSIM_F16_TWIN(launcher(args)); }.  DSIM_ERR_INVALID for anything else.
template <typename F, typename Twin>
int by_h16_dtype(int dtype, F&& f, Twin&& twin) {
    if (dtype == DSIM_H16) return f(Elem<h16>{});
#ifndef DSIM_H16_IS_F16
    if (dtype == DSIM_F32) return f(Elem<float>{});
    if (dtype == DSIM_F16) return twin();
#endif
    return DSIM_ERR_INVALID;
}

// parts of a workspace start on 256-byte boundaries
static inline size_t up256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// ---------------------------------------------------------------------------------------------
// implicit-GEMM (linear / 1x1 conv / 3x3 conv) -- gemm.hip
//   out[m][n] = epi( sum_k A(m,k) * W[n][k] + bias[n] )
// A is gathered on the fly from token-major activations:
//   LINEAR : A(m,k) = k < C0 ? A0[m*C0 + k] : A1[m*C1 + (k-C0)]      (channel concat of two sources)
//   CONV3  : k = tap*C0 + c ; A(m,k) = X[b][iy][ix][c], zero outside, optional stride 2 /
//            nearest-2x upsample folded into the index
// ---------------------------------------------------------------------------------------------
enum GemmMode { GEMM_LINEAR = 0, GEMM_CONV3 = 1, GEMM_CONV3P = 2 };   // CONV3P: gemm_kernel's instantiation for power-of-two output maps (never in GemmArgs.mode)
enum GemmEpi { EPI_NONE = 0, EPI_RESIDUAL = 1, EPI_GEGLU = 2 };
// gemm_kernel's compile-time epilogue kinds (what they are and why compile-time: gemm.hip, at the kernel)
enum { EK_PLAIN = 0, EK_RES = 1, EK_SLOW = 2, EK_ACT = 3,     // EK_ACT: tanh-GELU only (DiT Mlp.fc1): no gate, no residual registers
       EK_PLAIN_GN = 4, EK_RES_GN = 5 };                        // + GroupNorm statistics of the output from the read-back (GemmArgs.gn_part)

struct GemmArgs {
    const void* A0 = nullptr;
    const void* A1 = nullptr;
    int C0 = 0, C1 = 0;
    int mode = GEMM_LINEAR;
    int Hin = 0, Win = 0, Hout = 0, Wout = 0;   // CONV3 geometry (Hin/Win = stored input size)
    int stride = 1, ups = 0;
    int pad = 1;                                // 1: symmetric padding; 0: VAE downsample (pad right/bottom only)
    int lwo = -1, lhw = -1;                     // filled by launch_gemm: log2(Wout), log2(Hout * Wout) when both are powers of two, else -1
    int M = 0, N = 0, K = 0;                    // N counts packed weight rows (2x out cols for GEGLU)
    const void* W = nullptr;                    // packed [N][K], compute dtype
    const float* bias = nullptr;                // [N] f32 (packed order) or null
    const float* bias2 = nullptr;               // optional: bias of ODD batch elements (m / rows_per_batch) & 1 -- SDXL's
    int rows_per_batch = 0;                     //   time embedding differs between the uncond/cond CFG halves
    int act = 0;                                // 1: tanh-GELU after the bias (DiT Mlp.fc1)
    const float* gate = nullptr;                // optional per-column scale applied before the residual add (DiT adaLN
    const float* gate2 = nullptr;               //   gates); gate2 = the ODD batch elements' vector
    int epi = EPI_NONE;
    int geglu_blk = 32;                         // EPI_GEGLU: rows per alternating [h | g] block of the packed weight (geglu_block_rows())
    const void* residual = nullptr;             // [M][ldo]
    void* out = nullptr;
    int ldo = 0;
    int out_split = 0;                          // > 0 (plain linear only, % 320 == 0): output columns [j*split, (j+1)*split) go to the
    long long out_split_stride = 0;             //   tensor at out + j * out_split_stride bytes, each [M][ldo] (the tapped q | k | v)
    int force_big = 0;                          // 1: 256-row tiles whatever the tile count (a caller that needs the SAME tiles at every batch size:
                                                //    the VAE's 128 x 128 level asks for epilogue statistics, whose partial sums follow the tile shape)
    int wb_rows = 0;                            // optional (GEMM_LINEAR): batched weights -- rows [i * wb_rows, (i + 1) * wb_rows) multiply the
    unsigned wb_stride = 0;                     //   [N][K] matrix at W + i * wb_stride bytes (the VAE's per-image q k^T and P v); M % wb_rows == 0
    float* gn_part = nullptr;                   // optional (16-bit 3x3 convs on 256 x 128 / 256 x 256 tiles): GroupNorm statistics of the OUTPUT from
    int gn_hw = 0;                              //   the epilogue: [image][gn_hw / 64][N / 4][2] f32 (sum, sum of squares) per (wave's 64 rows, 4-channel
                                                //   quad); gn_hw = rows per image (% 256 == 0).  launch_groupnorm_pre folds them.
    const void* zero_page = nullptr;            // >= 16 zero bytes (kept for ABI stability; padding now comes from OOB buffer reads)
    unsigned a0_bytes = 0, a1_bytes = 0, w_bytes = 0, out_bytes = 0;   // filled by launch_gemm: operand extents for the buffer descriptors
#ifdef DSIM_DEVTOOLS
    int exp = 0;                                // kernel experiments (tools/kbench)
    unsigned long long* stamps = nullptr;       // -DDSIM_STAMPS builds: per-phase cycle sums of gemm_kernel (7 words)
#endif
};
// One gemm_kernel / gemm_skinny_kernel (small = 1) instantiation: tile, GemmMode (GEMM_CONV3P included), GEGLU, epilogue kind EK_*.
// gemm_plan() fills one for a problem: the plan launch_gemm follows and gemm_family(), gemm_gn_stats_tile() and tools/kbench read.
struct GemmLaunchRec {
    int bm = 0, bn = 0, mode = -1, geglu = 0, ek = -1, small = 0;
};
// The instantiation the calling thread's last GEMM launch ran, written by launch_ek / launch_skinny_t from their template parameters
// (one definition, in pack.hip, shared by the bf16 and fp16 objects): what dsim_op_gemm reports, so that tests see the kernel that ran.
extern thread_local GemmLaunchRec g_gemm_last_launch;
// Rows per alternating block of a GEGLU-interleaved weight with N packed rows (= 8C): 16 where the 320 / 160-column GEMM tiles
// divide N (their waves hold 160 or 80 packed rows: five or ten 16-row accumulator tiles, an odd count of 32-row blocks); 32 for
// the 320-channel blocks, whose weights the fused feed-forward streams (32 x 32 MFMAs), and for widths the 256 / 128-column tiles serve.
inline int geglu_block_rows(int N) { return (N % 320 == 0 && N != 8 * 320) ? 16 : 32; }
// Development switches (kernel A/B in tools/kbench, environment overrides): they exist only in -DDSIM_DEVTOOLS builds
// (tools/build_kbench.py); the product library compiles them away as constants.
#ifdef DSIM_DEVTOOLS
extern int g_gemm_persistent;   // 0 = one tile per workgroup
extern int g_force_bm;          // 0 = heuristic; 128/256 force the row tile
extern int g_gemm_exp;          // experiment mask passed to gemm_kernel
extern int g_gemm_skinny;       // 0 = small problems through gemm_kernel as well
extern unsigned long long* g_gemm_stamps;   // device buffer of gemm_kernel's phase stamps (-DDSIM_STAMPS builds)
extern int g_skinny_tile;       // 0 = heuristic, else (bm << 8) | bn
extern int g_attn_dbg;          // ablation mask of attn_long_kernel
extern float* g_tail160_dbg;    // kbench: device buffer for the first unit's two attention outputs
extern int g_tail160_exp;       // kbench: experiment mask of pair_tail160_kernel
extern int g_ff_dbg;            // ablation mask of the fused feed-forward kernel (rowres.hip)
extern int g_rl_dbg;            // ablation mask of the row-resident Linear kernel (rowres.hip)
extern int g_rl_wpc;            // rowlin_kernel's persistent workgroups per CU (kbench occupancy probe; the product's 3)
extern int g_ff_stagger;        // the feed-forward kernel's wave de-phasing, in s_nop 7 units per wave index; -1 = the product default
#else
constexpr int g_gemm_skinny = 1, g_gemm_persistent = 1, g_force_bm = 0, g_gemm_exp = 0, g_skinny_tile = 0;
constexpr int g_rl_wpc = 3, g_ff_stagger = -1;
#endif
// The small-batch kernel's tiles, by bm + bn: gemm_skinny.hip compiles exactly these, gemm_plan() (gemm.hip) tries the first
// kSkinnyChoices in this order
constexpr int kSkinnyTiles[][2] = {{64, 64}, {64, 80}, {64, 128}, {128, 80}, {128, 128},
#ifdef DSIM_DEVTOOLS
                                   {128, 64}, {128, 160},      // kbench sweep only (g_skinny_tile): never the heuristic's choice
#endif
};
constexpr int kSkinnyChoices = 5, kSkinnyCompiled = sizeof(kSkinnyTiles) / sizeof(kSkinnyTiles[0]);
// weight repack kernels -- pack.hip  (src f32/h16/f16 diffusers layout -> packed compute dtype)
int pack_linear(const void* src, int src_dtype, void* dst, int dst_dtype, int N, int K,
                int geglu_interleave, hipStream_t s);                       // [N][K] -> [N][K]; geglu_interleave: 0 or the block rows (16 / 32)
int pack_conv3(const void* src, int src_dtype, void* dst, int dst_dtype, int Cout, int Cin,
               hipStream_t s);                                              // [Co][Ci][3][3] -> [Co][9][Ci]
int pack_conv_in(const void* src, int src_dtype, float* dst, int Cout, int Cin, hipStream_t s);   // -> f32 [9*Ci][Co]
int pack_vector(const void* src, int src_dtype, float* dst, int N, int geglu_interleave,
                hipStream_t s);                                             // any -> f32
// y[n] = bias[n] + sum_k W[n][k] * act(x[k]) ; all f32, W may be f32/h16/f16 ; act: 0 id, 1 silu
int gemv_f32(const void* W, int w_dtype, const void* bias, int b_dtype, const float* x, float* y,
             int N, int K, int act, hipStream_t s);
int add_vectors_f32(const float* a, const float* b, float* out, int N, hipStream_t s);
int timestep_sincos(float* out, int dim, int t, hipStream_t s);
int sincos_values(float* out, int dim, const float* vals /*device*/, int count, hipStream_t s);

// noising + CFG duplication + conv_in (direct) -- pack.hip
//   x_t = sa*lat + sb*noise ; out[(img*2+cfg)][pix][co] for cfg in {0,1}
int prep_conv_in(const float* lat, const float* noise /*nullable*/, float sa, float sb, const float* w /*[9*Cin][Cout]*/,
                 const float* bias, void* out, int dtype, int n_img, int Cin, int S, int Cout, int dup /*1|2*/,
                 hipStream_t st);
// which direct kernel prep_conv_in launches, the one host decision: the eight-wide kernel where Cout % 8 == 0, Cout <= 2048 and its
// staging buffer fits 48 KB, else the generic one.  prep_conv_in_as launches the named kind (DSIM_ERR_INVALID where it does not apply)
enum { CONV_IN_GENERIC = 1, CONV_IN_EIGHT = 2, CONV_IN_ROWS = 3 };      // prep_conv_in_kernel, prep_conv_in8_kernel, conv_in_rows_kernel
bool prep_conv_in_kind_applies(int kind, int Cin, int Cout);
int prep_conv_in_kind(int Cin, int Cout);
int prep_conv_in_as(int kind, const float* lat, const float* noise, float sa, float sb, const float* w, const float* bias, void* out,
                    int dtype, int n_img, int Cin, int S, int Cout, int dup, hipStream_t st);
// the VAE's 3 -> 128 conv_in at image resolution, one 64-pixel row segment per workgroup (bit-identical to prep_conv_in); gn_part
// (16-bit dtypes only, nullable): the consumer's GroupNorm statistics in the conv epilogue's format (launch_groupnorm_pre)
bool conv_in_rows_applies(int Cin, int S, int Cout);
int conv_in_rows(const float* images, const float* w /*[27][128]*/, const float* bias, void* out, int dtype, int n_img, int S,
                 float* gn_part, hipStream_t st);
int convert_f32_to(const float* src, void* dst, int dtype, size_t n, hipStream_t s);
// per-element prompt contexts: dst[(2 img + cfg)][per] = ctx[clamp(index[img], 0, n_ctx - 1)][cfg][per] in the compute dtype, each
// value converted as convert_f32_to converts it (ctx f32 [n_ctx][2][per], index int32 device [n_images], per = ctx_len * Dc)
int gather_ctx(const float* ctx, int n_ctx, const int32_t* index, void* dst, int dtype, int n_images, size_t per, hipStream_t s);
// out[2b], out[2b+1] = in[b]: a batch element becomes its two classifier-free-guidance copies (bytes_per_elem % 16 == 0)
int dup_batch(const void* in, void* out, int n_batch, size_t bytes_per_elem, hipStream_t s);
// token-major nearest-neighbour resize [B][Hin][Win][C] -> [B][Hout][Wout][C] (row_bytes = C * element size, % 16 == 0), source
// index = min(floor(dst * (float)in / out), in - 1) as F.interpolate(mode="nearest") computes it: the explicit-size
// upsample of latent sides that are not a multiple of 2**levels (diffusers' forward_upsample_size)
int resize_nearest(const void* in, void* out, int B, int Hin, int Win, int Hout, int Wout, size_t row_bytes, hipStream_t s);

// DiT's patch embedding -- dit.hip: x_t = sa * lat + sb * noise (NCHW f32 [n_img][Cin][S][S]), the p x p patch projection with
// w f32 [D][Cin p p], + bias + pos [T][D], written to both CFG halves out[(img * 2 + cfg)][T][D], T = (S / p)^2
int patch_embed(const float* lat, const float* noise, float sa, float sb, const float* w, const float* bias, const float* pos, void* out,
                int dtype, int n_img, int Cin, int S, int p, int D, hipStream_t s);
// the VAE's quant_conv folded into conv_out -- vae.hip: out_w[Cm][K] = wq[Cm][Cm] wco[Cm][K] (wco / out_w in the compute dtype, wq f32),
// out_b = wq bco + bq (f32; one workgroup of up to 1024 threads: Cm beyond that is DSIM_ERR_INVALID); either half may be left out
// (out_w or out_b null)
int fold_quant(const float* wq, const void* wco, const float* bco, const float* bq, void* out_w, float* out_b, int Cm, int K, int dtype,
               hipStream_t s);
// token-major [n][HW][C] in the compute dtype -> f32 NCHW [n][C][HW] -- vae.hip
int to_nchw_f32(const void* x, float* out, int n, int HW, int C, int dtype, hipStream_t s);

// row-resident Linear for K = 320 and 640: out[M][N] = P(x) W^T (+ bias), N % 64 == 0, N <= 3 C -- rowres.hip.  P: nothing, a
// LayerNorm (ln_g, ln_b), or -- the GroupNorm form, gn = 1, N <= C -- the per-image channel affine of launch_groupnorm_stats' table
struct RowLinArgs {
    const void* x = nullptr;                    // [M][C] h16
    void* out = nullptr;                        // [M][N] h16
    const float* ln_g = nullptr;                // null: no LayerNorm in front
    const float* ln_b = nullptr;
    const void* stream = nullptr;               // pack_rowlin_stream output
    int M = 0, C = 0, N = 0;
    float eps = 1e-5f;
    int dtype = DSIM_BF16;                      // DSIM_BF16 or DSIM_F16
    int gn = 0;                                 // the GroupNorm form: the two below, no LayerNorm
    const float* coef = nullptr;                // [M / HW][2][C] f32 (sc, sh per image and channel); null: x enters as it is
    const float* bias = nullptr;                // [N] f32, the accumulators' initial value; null: none
    int HW = 0;                                 // rows per image (coef: HW % 128 == 0, M % HW == 0)
};

// uint8 HWC pixels -> process_image's normalised NCHW f32 (half: rounded through fp16); VAE posterior sample -- pack.hip
int image_preprocess(const unsigned char* hwc, float* out, int n, int H, int W, int half, hipStream_t s);
int latent_sample(const float* moments, const float* eps, float* out, int n_out, int first, int stride, int C, int hw, int eps_n,
                  float sf, int round16, hipStream_t s);

// norms -- norm.hip
size_t groupnorm_scratch_bytes(int B, int groups);
int groupnorm_passes(int C0, int C1, int HW, int groups, int dtype);    // 2 (one-pass form) or 3: algorithmic tensor passes
// the dispatch of launch_groupnorm / launch_groupnorm_pre (pre = 1) and launch_layernorm / launch_layernorm_mod (mod = 1): the
// function the launchers themselves call; host only, DSIM_ERR_INVALID where the launch would refuse the shape
int groupnorm_plan(int C0, int C1, int B, int HW, int groups, int dtype, int pre, dsim_gn_plan* plan);
int layernorm_plan(int M, int C, int dtype, int mod, dsim_ln_plan* plan);
int launch_groupnorm(const void* x0, int C0, const void* x1, int C1, const float* gamma,
                     const float* beta, void* out, int B, int HW, int groups, float eps, int silu,
                     int dtype, void* scratch, hipStream_t s);
int launch_groupnorm_pre(const void* x, int C, const float* gamma, const float* beta, void* out, int B, int HW, int groups, float eps,
                         int silu, int dtype, void* scratch, const float* part32, int chunks, hipStream_t s);   // statistics from GemmArgs.gn_part
// The statistics-only GroupNorm (16-bit dtypes): launch_groupnorm's statistics for this shape (same scratch) and no apply pass; coef =
// the caller's table [B][2][C] f32 (16-byte aligned), (sc, sh) with y = fmaf(x, sc, sh) the bits launch_groupnorm writes (RowLinArgs.coef)
int launch_groupnorm_stats(const void* x, int C, const float* gamma, const float* beta, int B, int HW, int groups, float eps, int dtype,
                           void* scratch, float* coef, hipStream_t s);
int launch_layernorm(const void* x, const float* gamma, const float* beta, void* out, int M, int C,
                     float eps, int dtype, hipStream_t s);
// LayerNorm without affine followed by adaLN modulate: y = LN(x) * (1 + scale[half]) + shift[half], half =
// (row / rows_per_batch) & 1 (DiT blocks; scale/shift are f32 [2][C])
int launch_layernorm_mod(const void* x, const float* scale2, const float* shift2, void* out, int M, int C,
                         int rows_per_batch, float eps, int dtype, hipStream_t s);
// out[r][:] = softmax(x[r][:] * scale) over `cols` (VAE mid-block attention; in place allowed)
int launch_softmax_rows(const void* x, void* out, int rows, int cols, float scale, int dtype, hipStream_t s);

// attention -- attention.hip (its tiled core, which the score tails of tails.hip share: attn_core.h)
struct AttnArgs {
    const void* q = nullptr; int ldq = 0;     // [B][Nq] rows of ldq elements, head h at column h*D
    const void* k = nullptr; const void* v = nullptr; int ldk = 0;   // [Bkv][Nk] rows
    void* out = nullptr; int ldo = 0;
    int B = 0, Bkv = 0, H = 0, Nq = 0, Nk = 0, D = 0;
    int xcd_remap = 1;                        // 0: plain block order (micro-benchmark A/B only)
};
// The kernels launch_attention starts (attention.hip attention_kernel() picks one), numbered as include/diffsim_amd.h's dsim_attn_kind;
// profile family suffixes as attn_kind_suffix() names them (bench.py maps family names to the symbols rocprofv3 prints):
enum class AttnKernel {
    P160 = DSIM_ATTN_P160,          // "_p160"   sdpa160_kernel (attn160.hip): 256 x 256 tokens at d = 160 on the persistent core
    Short = DSIM_ATTN_SHORT,        // "_short"  attn_short_kernel<D, false>: keys resident in LDS
    ShortK80 = DSIM_ATTN_SHORT_K80, // "_short"  attn_short_kernel<D, true>: the same for 64 < Nk <= 80 (the 77-key prompt context)
    Long = DSIM_ATTN_LONG,          // "_long"   attn_long_kernel: two query blocks per wave, pipelined
    Q2 = DSIM_ATTN_Q2,              // "_q2"     attn_q2_kernel<D, false>: two query blocks per wave sharing every fragment read, exact softmax
    Q2Fast = DSIM_ATTN_Q2FAST,      // "_q2fast" attn_q2_kernel<D, true>: the same with the fixed-reference softmax
    Fast = DSIM_ATTN_FAST,          // "_fast"   attn_kernel<T, D, true>: the fixed-reference softmax
    Exact = DSIM_ATTN_EXACT,        // ""        attn_kernel<T, D, false>: the exact running maximum
};
inline const char* attn_kind_suffix(int kind) {
    switch (kind) {
        case DSIM_ATTN_P160: return "_p160";
        case DSIM_ATTN_SHORT:
        case DSIM_ATTN_SHORT_K80: return "_short";
        case DSIM_ATTN_LONG: return "_long";
        case DSIM_ATTN_Q2: return "_q2";
        case DSIM_ATTN_Q2FAST: return "_q2fast";
        case DSIM_ATTN_FAST: return "_fast";
        default: return "";
    }
}
// The attention kernel the calling thread launched last, written where launch_attn_d / launch_sdpa160 / launch_attention_fp8 launch it
// (one definition, in pack.hip, shared by the bf16 and fp16 objects): what dsim_op_attention_ex reports, so that tests see the kernel
// that ran rather than the one the dispatch rule names.
struct AttnLaunchRec {
    int kind = -1, D = 0, dtype = -1, k80 = 0, qit = 0, grid = 0;
};
extern thread_local AttnLaunchRec g_attn_last_launch;
int launch_attention_fp8(const AttnArgs& a, hipStream_t s);      // h16 in/out, e4m3 MFMAs (attention_fp8.hip)

// the score tails over pairs of feature images -- tails.hip, regions.hip, align.hip, attn160.hip: what launch_pair_score, _maps,
// _regions, _align and launch_pair_score160 share; their outputs and the compute dtype travel beside it
struct PairArgs {
    const void* q = nullptr;                    // q, k, v: [n_feat][B][N][H*D] contiguous, the compute dtype (v: unused by the
    const void* k = nullptr;                    //   alignments)
    const void* v = nullptr;
    const int32_t* idx_a = nullptr;             // device [n_pairs] each: pair p is (image idx_a[p], image idx_b[p])
    const int32_t* idx_b = nullptr;
    int n_pairs = 0, B = 0, H = 0, N = 0, D = 0;
    int similarity = 0;                         // 0 cosine, 1 mse
    void* scratch = nullptr;                    // 256-byte aligned; the launcher's *_scratch_bytes
    size_t scratch_bytes = 0;
};

// the score matrices over two sets of feature images -- tails.hip, region_matrix.hip, attn160.hip: what launch_score_matrix,
// _matrix160 and _matrix_regions share; their outputs and the compute dtype travel beside it
struct MatrixArgs {
    const void* q[2];                           // set A, set B, each q, k, v: [n][B][N][H*D] contiguous, the compute dtype
    const void* k[2];
    const void* v[2];
    const uint8_t* mask[2];                     // device [n][N] bytes per set, non-zero = on; both null: the unmasked call
    int n_a, n_b, B, H, N, D;
    int similarity;                             // 0 cosine, 1 mse
    void* scratch;                              // 256-byte aligned; the launcher's *_scratch_bytes
    size_t scratch_bytes;
};

// row-resident fused feed-forward of the 320-channel transformer blocks (h16) -- rowres.hip
//   out = x + W2 (h * gelu(g)) + b2,  [h ; g] = W1 LN(x) + b1
struct FFArgs {
    const void* x = nullptr;                    // [M][C] h16: LayerNorm input and residual
    void* out = nullptr;                        // [M][C] h16 (may alias x)
    const float* ln_g = nullptr;
    const float* ln_b = nullptr;
    const void* stream = nullptr;               // pack_ff_stream output
    const float* b1 = nullptr;                  // [8C] f32, GEGLU-interleaved (pack_vector with geglu_interleave = 1)
    const float* b2 = nullptr;                  // [C] f32
    int M = 0, C = 0;
    float eps = 1e-5f;
    int dtype = DSIM_BF16;                      // DSIM_BF16 or DSIM_F16
};

// The entry points of the sources compiled once per 16-bit type, in this compilation's own namespace ...
inline namespace DSIM_H16_NS {
#include "h16_api.h"
// Can launch_gemm take GemmArgs.gn_part for this problem?  (16-bit 3x3 conv on a power-of-two output map whose tile has a
// statistics epilogue, N a multiple of it, whole tiles per image: the plan's answer with gn_part asked for.)  The executors ask with
// the geometry of ONE image: where a single image already fills the chip's tiles, every batch size runs the same tiles and the
// statistics are batch-invariant.
inline bool gemm_gn_stats_tile(const GemmArgs& a, int dtype) {
    if (dtype == DSIM_F32 || a.mode != GEMM_CONV3 || a.epi == EPI_GEGLU || a.bias2 || a.Wout <= 0) return false;
    const int hw = a.Hout * a.Wout;
    if ((a.Wout & (a.Wout - 1)) || (hw & (hw - 1)) || hw % 256) return false;
    float asked = 0.f;                          // (the plan reads gn_part and zero_page as flags, never through them)
    GemmArgs q = a;
    q.gn_part = &asked; q.gn_hw = hw; q.zero_page = &asked;
    GemmLaunchRec plan;
    return gemm_plan(q, dtype, &plan) == DSIM_OK;
}
// The refusals every pair launcher makes before its own (DSIM_ERR_INVALID): a dtype outside the three, a similarity outside 0 | 1, a
// shape pair_shape_served refuses.  tiled = false: a persistent launch, whose grid carries B*H on no axis.
inline int pair_args_check(const PairArgs& a, int dtype, bool tiled = true) {
    if (dtype != DSIM_F32 && dtype != DSIM_BF16 && dtype != DSIM_F16) return DSIM_ERR_INVALID;
    if (a.similarity != 0 && a.similarity != 1) return DSIM_ERR_INVALID;
    return pair_shape_served(a.n_pairs, a.B, a.H, a.N, a.D, tiled) ? DSIM_OK : DSIM_ERR_INVALID;
}
// The same for the matrix launchers: a similarity outside 0 | 1, a call matrix_shape_served refuses (listed: the region matrix)
inline int matrix_args_check(const MatrixArgs& a, int dtype, bool listed) {
    if (a.similarity != 0 && a.similarity != 1) return DSIM_ERR_INVALID;
    return matrix_shape_served(a.n_a, a.n_b, a.B, a.H, a.N, a.D, dtype, listed) ? DSIM_OK : DSIM_ERR_INVALID;
}
}  // namespace DSIM_H16_NS
// ... and, seen from the bf16 objects of the product build, their fp16 twins: DSIM_F16_TWIN(f(args)) is how a bf16 launcher forwards
// compute dtype DSIM_F16.  tools/kbench (-DDSIM_DEVTOOLS) links no second compilation: there, as in the fp16 objects themselves,
// which have nothing to forward, the call is DSIM_ERR_INVALID.
#if !defined(DSIM_H16_IS_F16) && !defined(DSIM_DEVTOOLS)
namespace f16 {
#include "h16_api.h"
}
#define DSIM_F16_TWIN(call) f16::call
#else
#define DSIM_F16_TWIN(call) DSIM_ERR_INVALID
#endif

// Per-device once-flags for hipFuncSetAttribute(MaxDynamicSharedMemorySize) and the CU count (one cache, in pack.hip): the
// attribute is a per-device property of the function, so a process that drives several devices must set it on each.
int cu_count();
struct DeviceOnce {
    unsigned long long done = 0;       // bit d set: attribute applied on device d (d < 64)
    template <typename F> int ensure(F&& apply) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return DSIM_ERR_HIP;
        if (dev >= 0 && dev < 64 && (__atomic_load_n(&done, __ATOMIC_ACQUIRE) >> dev) & 1ull) return DSIM_OK;
        const int st = apply();          // idempotent: two racing threads may both apply it
        if (st == DSIM_OK && dev >= 0 && dev < 64) __atomic_fetch_or(&done, 1ull << dev, __ATOMIC_RELEASE);
        return st;
    }
};
// The one way a kernel with opted-in dynamic LDS is launched: Kern's once-flag (one per instantiation, so one per kernel), the
// attribute, the launch and its error check.  DSIM_OK means the kernel is in the stream; launch records are written after it.
template <auto Kern, typename... A>
int launch_lds(dim3 grid, dim3 block, int lds_bytes, hipStream_t s, A... args) {
    static DeviceOnce once;
    const int st = once.ensure([&]() -> int {
        return hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) == hipSuccess ? DSIM_OK
                                                                                                                            : DSIM_ERR_HIP;
    });
    if (st != DSIM_OK) return st;
    hipLaunchKernelGGL(Kern, grid, block, lds_bytes, s, args...);
    return hipGetLastError() == hipSuccess ? DSIM_OK : DSIM_ERR_HIP;
}

}  // namespace dsim
