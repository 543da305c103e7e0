// VGG executor (normalised pixels -> the last conv's output, channel-last) and the Gram rows of channel-last features, with their C
// ABI: the backbone of the reference's `gram` metric (metrics/vgg_gram.py: torchvision vgg19().features up to module '28', conv5_1
// before its ReLU; G = X X^T over the spatial axis; the cosine of two Gram rows or matrices).
// Graph: a plan of 3x3 convs (stride 1, padding 1, bias) and 2x2 max-pools (stride 2, floor mode); a ReLU follows every conv but the
// last, whose output is the tap.  One call is one batch of equally sized images, H and W independent and of any parity.
// Kernels:
//  * vgg_conv_first_kernel: the first conv, straight from the f32 NCHW pixels (Cin = 3: K = 27, which the implicit GEMM's K tile does
//                           not divide), one pixel and 8 output channels per thread, the workgroup's 8 filters in LDS.
//  * the implicit-GEMM 3x3 conv of gemm.hip with its bias epilogue for every other conv, unchanged.
//  * relu_kernel / relu_pool2_kernel: 16-byte channel segments; the pool reads rows 2y, 2y + 1 and columns 2x, 2x + 1 of its output
//                           pixels only, so an odd last row or column is never touched.  NaN goes through both (torch's semantics).
//  * gram_mfma_kernel:      G[r][c] = sum_p X[p][r] X[p][c] for 16-bit X on the matrix cores: 32 rows x 128 columns per workgroup (a
//                           32 x 32 MFMA tile per wave), 32 positions per stage.  BOTH operands are the transposed-A kind: a stage is
//                           two plain channel-last images in LDS (the row block's 32 channels, 64-byte rows; the column block's 128
//                           channels, 256-byte rows padded to 320) and every fragment is a ds_read_b64_tr_b16 pair.  A 32-lane half
//                           reads 4 rows x 64 bytes: with row strides of 64 and 320 bytes (16 dwords mod 64) the four rows fall on
//                           four disjoint 16-bank ranges, so the transposed reads are conflict-free.  The two operands take the
//                           same positions in the same fragment slots, so the order of p inside a fragment does not matter.
//                           4 waves and 24 KB of LDS per workgroup: occupancy is bound by neither (an 8-wave workgroup would halve
//                           the LDS traffic per MFMA of the row operand only, which is the small one).
//  * gram_vec_kernel:       the same sum on the vector unit, one output per thread: f32 features, and a few rows (n_rows < 8 or a
//                           row0 off the 8-channel grid; the reference's single row).
//  * gram_fold_kernel / gram_stats_kernel: P is split over workgroups in GRAM_PCHUNK positions; the f32 partials fold in ascending p
//                           order; per image (sum of squares in f64, min, max) in a fixed order.  No atomics.
// An image's activations, Gram rows and stats do not depend on the other images of the call beyond the GEMM tile choice.
#include <string>
#include <vector>

#include "common.h"
#include "store.h"

using namespace dsim;

struct dsim_vgg : WeightStore {
    dsim_vgg_cfg cfg;
    int n_plan = 0;             // entries before the terminator
};

namespace {

constexpr int V16 = 16;         // bytes per thread and access of the element-wise kernels
template <typename T> struct VecOf { typedef T type __attribute__((ext_vector_type(V16 / sizeof(T)))); };

inline unsigned ew_blocks(size_t groups) {
    const size_t b = (groups + 255) / 256;
    return (unsigned)(b < 65536 ? (b ? b : 1) : 65536);
}

// NaN-propagating ReLU and maximum (torch.relu, F.max_pool2d)
__device__ __forceinline__ float relu_f(float x) { return x < 0.f ? 0.f : x; }
__device__ __forceinline__ float max_nan(float m, float b) { return (b > m || b != b) ? b : m; }

// x[i] = relu(x[i]) in place, groups of 16 bytes
template <typename T>
__global__ __launch_bounds__(256) void relu_kernel(T* __restrict__ x, size_t groups) {
    constexpr int VEC = V16 / sizeof(T);
    typedef typename VecOf<T>::type Vec;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < groups; i += (size_t)gridDim.x * 256) {
        Vec v = *(const Vec*)(x + i * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = (T)relu_f((float)v[e]);
        *(Vec*)(x + i * VEC) = v;
    }
}

// out [n][H/2][W/2][C] = max over the 2x2 window of relu(in [n][H][W][C]); groups = n (H/2) (W/2) C / VEC
template <typename T>
__global__ __launch_bounds__(256) void relu_pool2_kernel(const T* __restrict__ in, T* __restrict__ out, int H, int W, int C, size_t groups) {
    constexpr int VEC = V16 / sizeof(T);
    typedef typename VecOf<T>::type Vec;
    const int Ho = H / 2, Wo = W / 2, cg = C / VEC;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < groups; i += (size_t)gridDim.x * 256) {
        const size_t pix = i / cg;
        const int c0 = (int)(i - pix * cg) * VEC;
        const size_t row = pix / Wo, img = row / Ho;
        const int ox = (int)(pix - row * Wo), oy = (int)(row - img * Ho);
        const T* src = in + ((img * H + 2 * oy) * W + 2 * ox) * C + c0;
        const Vec a = *(const Vec*)src, b = *(const Vec*)(src + C);
        const Vec c = *(const Vec*)(src + (size_t)W * C), d = *(const Vec*)(src + (size_t)W * C + C);
        Vec v;
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            v[e] = (T)relu_f(max_nan(max_nan((float)a[e], (float)b[e]), max_nan((float)c[e], (float)d[e])));
        *(Vec*)(out + i * VEC) = v;
    }
}

// out [n][H][W][Cout] = conv3x3(pix f32 [n][CIN][H][W], padding 1) + bias, w [Cout][9][CIN] in the compute dtype (pack_conv3's layout).
// grid (pixel blocks, Cout / 8): the 8 output channels of a workgroup share their weights, staged once in LDS as f32.
template <typename T, int CIN>
__global__ __launch_bounds__(256) void vgg_conv_first_kernel(const float* __restrict__ pix, const T* __restrict__ w,
                                                             const float* __restrict__ bias, T* __restrict__ out, int H, int W, int Cout,
                                                             size_t pixels) {
    constexpr int K = 9 * CIN;
    typedef T Vec8 __attribute__((ext_vector_type(8)));
    const int co0 = blockIdx.y * 8;
    const size_t hw = (size_t)H * W;
    __shared__ float ws[8 * K];         // the workgroup's 8 filters in f32: every lane reads the same word (a broadcast)
    for (int j = threadIdx.x; j < 8 * K; j += 256) ws[j] = (float)w[(size_t)co0 * K + j];
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (size_t)gridDim.x * 256) {
        const size_t img = i / hw, rem = i - img * hw;
        const int y = (int)(rem / W), x = (int)(rem - (size_t)y * W);
        float in[K];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
            const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) in[t * CIN + ci] = ok ? pix[((img * CIN + ci) * H + yy) * W + xx] : 0.f;
        }
        Vec8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float acc = bias[co0 + e];
#pragma unroll
            for (int k = 0; k < K; ++k) acc = fmaf(in[k], ws[e * K + k], acc);
            v[e] = (T)acc;
        }
        *(Vec8*)(out + i * Cout + co0) = v;
    }
}

int launch_relu(void* x, size_t elems, int dtype, hipStream_t s) {
    return by_dtype(dtype, [&](auto e) -> int {
        typedef typename decltype(e)::type T;
        const size_t groups = elems / (V16 / sizeof(T));
        hipLaunchKernelGGL(relu_kernel<T>, dim3(ew_blocks(groups)), dim3(256), 0, s, (T*)x, groups);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

int launch_relu_pool2(const void* in, void* out, int n, int H, int W, int C, int dtype, hipStream_t s) {
    return by_dtype(dtype, [&](auto e) -> int {
        typedef typename decltype(e)::type T;
        const size_t groups = (size_t)n * (H / 2) * (W / 2) * C / (V16 / sizeof(T));
        hipLaunchKernelGGL(relu_pool2_kernel<T>, dim3(ew_blocks(groups)), dim3(256), 0, s, (const T*)in, (T*)out, H, W, C, groups);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

int launch_conv_first(const float* pix, const void* w, const float* bias, void* out, int n, int Cin, int H, int W, int Cout, int dtype,
                      hipStream_t s) {
    const size_t pixels = (size_t)n * H * W;
    const unsigned bx = ew_blocks(pixels);
    return by_dtype(dtype, [&](auto e) -> int {
        typedef typename decltype(e)::type T;
        const dim3 grid(bx < 32768 ? bx : 32768, Cout / 8);
        switch (Cin) {
            case 1: hipLaunchKernelGGL((vgg_conv_first_kernel<T, 1>), grid, dim3(256), 0, s, pix, (const T*)w, bias, (T*)out, H, W, Cout, pixels); break;
            case 2: hipLaunchKernelGGL((vgg_conv_first_kernel<T, 2>), grid, dim3(256), 0, s, pix, (const T*)w, bias, (T*)out, H, W, Cout, pixels); break;
            case 3: hipLaunchKernelGGL((vgg_conv_first_kernel<T, 3>), grid, dim3(256), 0, s, pix, (const T*)w, bias, (T*)out, H, W, Cout, pixels); break;
            case 4: hipLaunchKernelGGL((vgg_conv_first_kernel<T, 4>), grid, dim3(256), 0, s, pix, (const T*)w, bias, (T*)out, H, W, Cout, pixels); break;
            default: return DSIM_ERR_INVALID;
        }
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    });
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------------
struct VggWalk : WalkBase<dsim_vgg> {
    const int n;
    int Ho = 0, Wo = 0, Co = 0;     // the tap's geometry
    VggWalk(dsim_vgg* h, Arena* ar, hipStream_t s, int n, bool run) : WalkBase(h, ar, s, run), n(n) {}

    int go(const float* pix, int H, int W, void* out) {
        const dsim_vgg_cfg& c = h->cfg;
        const int np = h->n_plan;
        // the two ping-pong buffers hold every activation but the tap: the largest of them
        size_t biggest = 0;
        {
            int hh = H, ww = W;
            for (int i = 0; i < np; ++i) {
                if (c.plan[i] > 0) {
                    if (i + 1 < np && (size_t)n * hh * ww * c.plan[i] > biggest) biggest = (size_t)n * hh * ww * c.plan[i];
                } else {
                    hh /= 2; ww /= 2;
                    if (hh < 1 || ww < 1) return DSIM_ERR_INVALID;      // the image is smaller than the plan's pools
                }
            }
        }
        void* buf[2] = {alloc_act(biggest), alloc_act(biggest)};
        int cur = 0, conv = 0;
        Act x{nullptr, c.in_channels, H, W, n};
        for (int i = 0; i < np; ++i) {
            const int Cout = c.plan[i];
            const bool last = i + 1 == np;
            const std::string key = "convs." + std::to_string(conv++);
            WGET(cw, key + ".weight"); WGET(cb, key + ".bias");
            if (cw->rows != Cout || cw->cols != 9 * x.C || cb->rows != Cout) return DSIM_ERR_INVALID;
            void* y = last ? out : buf[cur ^ 1];
            if (i == 0) {
                CK(launch([&] { return rec(std::string("vgg_conv_first_") + dtn() + "|M" + std::to_string(x.rows()) + " N" + std::to_string(Cout) +
                                               " K" + std::to_string(9 * x.C), 2.0 * x.rows() * (double)Cout * 9 * x.C,
                                           (double)x.rows() * (4.0 * x.C + (double)Cout * es())); },
                          [&] { return launch_conv_first(pix, cw->p, (const float*)cb->p, y, n, x.C, x.H, x.W, Cout, h->dt, s); }));
            } else {
                GemmArgs g = conv3_args(x, cw->p, (const float*)cb->p, nullptr, y, Cout, 1, 0, 1);
                if (!run) {             // the plan's answer for this shape, before anything is launched
                    g.zero_page = h->zero_page;
                    GemmLaunchRec r;
                    CK(gemm_plan(g, h->dt, &r));
                } else {
                    CK(gemm(g));
                }
            }
            x = Act{y, Cout, x.H, x.W, n};
            cur ^= 1;
            if (last) break;
            if (c.plan[i + 1] == 0) {
                const Act in = x;
                void* p = buf[cur ^ 1];
                CK(launch([&] { return rec(std::string("relu_pool2_") + dtn() + "|M" + std::to_string(in.rows()) + " C" + std::to_string(Cout), 0.0,
                                           1.25 * in.rows() * (double)Cout * es()); },
                          [&] { return launch_relu_pool2(in.p, p, n, in.H, in.W, Cout, h->dt, s); }));
                x = Act{p, Cout, in.H / 2, in.W / 2, n};
                cur ^= 1;
                ++i;
            } else {
                CK(launch([&] { return rec(std::string("relu_") + dtn() + "|M" + std::to_string(x.rows()) + " C" + std::to_string(Cout), 0.0,
                                           2.0 * x.rows() * (double)Cout * es()); },
                          [&] { return launch_relu(x.p, (size_t)x.rows() * Cout, h->dt, s); }));
            }
        }
        Ho = x.H; Wo = x.W; Co = x.C;
        const size_t tap = (size_t)n * Ho * Wo * Co * es();
        if (tap > max_tensor) max_tensor = tap;
        return DSIM_OK;
    }
};

// dry walk: peak arena bytes and the tap's geometry; refuses a batch whose largest activation reaches 2 GiB (32-bit tensor offsets in
// the implicit GEMM) and one whose rows overflow an int
int vgg_plan(dsim_vgg* h, int n, int H, int W, size_t* peak, int* Ho, int* Wo, int* Co) {
    if (n < 1 || H < 1 || W < 1 || (size_t)n * H * W >= 0x7fffffffull) return DSIM_ERR_INVALID;
    Arena ar;
    VggWalk w{h, &ar, nullptr, n, false};
    CK(w.go(nullptr, H, W, nullptr));
    if (w.max_tensor >= 0x7fffffffull) return DSIM_ERR_INVALID;
    *peak = ar.peak;
    if (Ho) { *Ho = w.Ho; *Wo = w.Wo; *Co = w.Co; }
    return DSIM_OK;
}

// ---- Gram rows ---------------------------------------------------------------------------------------------------------------------
constexpr int GRAM_PCHUNK = 512;      // positions per workgroup (a multiple of a stage's 32)
constexpr int GR = 32, GC = 128;      // gram_mfma_kernel's tile: rows, columns
constexpr int GBK = 32;               // positions per stage
constexpr int GA_RS = 64, GB_RS = 320;                  // LDS row strides of the two images (bytes)
constexpr int GA_BYTES = GBK * GA_RS, G_STAGE = GA_BYTES + GBK * GB_RS;

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4_t;
template <typename T> struct Frag8;
template <> struct Frag8<bf16_t> { typedef bf16x8_t type; };
template <> struct Frag8<f16_t> { typedef f16x8_t type; };

// two transposed reads (rows r .. r + 3 and r + 8 .. r + 11 of the image at p, row stride rs) into one 32x32x16 operand
__device__ __forceinline__ bf16x8_t tr_frag(const char* p, int rs, bf16_t) {
    const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4_t*)(p));
    const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4_t*)(p + 8 * rs));
    bf16x8_t f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = lo[j]; f[4 + j] = hi[j]; }
    return f;
}
__device__ __forceinline__ f16x8_t tr_frag(const char* p, int rs, f16_t) {
    typedef __fp16 fp16v4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
    const f16x4_t lo = __builtin_bit_cast(f16x4_t, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16v4*)(p)));
    const f16x4_t hi = __builtin_bit_cast(f16x4_t, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16v4*)(p + 8 * rs)));
    f16x8_t f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[j] = lo[j]; f[4 + j] = hi[j]; }
    return f;
}
__device__ __forceinline__ void gram_mma(const bf16x8_t& a, const bf16x8_t& b, f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ void gram_mma(const f16x8_t& a, const f16x8_t& b, f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// part[img][split][r - row0][c] = sum over the split's positions of X[p][r] X[p][c].  X [n][P][C] (16-bit), C % 8 == 0, row0 % 8 == 0.
// grid (ceil(C / 128), ceil(n_rows / 32), n * splits).  Every lane runs every transposed read (EXEC all ones): positions past the
// split's end and channels past C are staged as zeros, outputs past the edges are dropped at the store.
template <typename T>
__global__ __launch_bounds__(256) void gram_mfma_kernel(const T* __restrict__ X, int P, int C, int row0, int n_rows, int splits,
                                                        float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) char lds[2 * G_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int img = blockIdx.z / splits, z = blockIdx.z - img * splits;
    const int pb = z * GRAM_PCHUNK, pe = (P - pb < GRAM_PCHUNK) ? P : pb + GRAM_PCHUNK;
    const int nkt = (pe - pb + GBK - 1) / GBK;
    const int r0 = row0 + blockIdx.y * GR, c0 = blockIdx.x * GC;
    const T* Xi = X + (size_t)img * P * C;
    // staging, 16-byte chunks of 8 channels: slots 0 and 1 are the column image's (position j / 16, chunk j % 16 of j = tid, tid + 256),
    // slot 2 the row image's (threads 0 .. 127: position tid / 4, chunk tid % 4)
    int sp[3], sch[3];
    bool ok[3];
    unsigned loff[3];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int j = tid + i * 256;
        sp[i] = j >> 4;
        sch[i] = c0 + (j & 15) * 8;
        ok[i] = sch[i] < C;
        loff[i] = (unsigned)(GA_BYTES + sp[i] * GB_RS + (j & 15) * 16);
    }
    sp[2] = (tid & 127) >> 2;
    sch[2] = r0 + (tid & 3) * 8;
    ok[2] = tid < 128 && sch[2] < C;
    loff[2] = (unsigned)(sp[2] * GA_RS + (tid & 3) * 16);
    u32x4 st[3];
    auto load = [&](int kt) {
        const int p0 = pb + kt * GBK;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const u32x4 zero = {0u, 0u, 0u, 0u};
            const int p = p0 + sp[i];
            st[i] = (ok[i] && p < pe) ? *reinterpret_cast<const u32x4*>(Xi + (size_t)p * C + sch[i]) : zero;
        }
    };
    // transposed read: per 16-lane group a 4 x 16 block; lane 4q + p' of the group supplies row q, columns 4p' .. 4p' + 3, and lane i
    // receives column i.  Groups 0, 1 (half 0) take rows 0 .. 3 (+ 8), groups 2, 3 rows 4 .. 7 (+ 8); the odd groups columns 16 .. 31.
    const int i16 = lane & 15, g = lane >> 4;
    const int trow = 4 * (g >> 1) + (i16 >> 2), tcol = 16 * (g & 1) + 4 * (i16 & 3);
    const int a_off = trow * GA_RS + tcol * 2;
    const int b_off = GA_BYTES + trow * GB_RS + (wave * 32 + tcol) * 2;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    load(0);
    for (int kt = 0; kt < nkt; ++kt) {
        // buffer (kt & 1) was last read in iteration kt - 2; every wave has passed barrier kt - 1 since
        char* buf = lds + (kt & 1) * G_STAGE;
        *reinterpret_cast<u32x4*>(buf + loff[0]) = st[0];
        *reinterpret_cast<u32x4*>(buf + loff[1]) = st[1];
        if (tid < 128) *reinterpret_cast<u32x4*>(buf + loff[2]) = st[2];
        __syncthreads();
        if (kt + 1 < nkt) load(kt + 1);
#pragma unroll
        for (int ks = 0; ks < GBK / 16; ++ks) {
            const auto af = tr_frag(buf + a_off + ks * 16 * GA_RS, GA_RS, T());
            const auto bf = tr_frag(buf + b_off + ks * 16 * GB_RS, GB_RS, T());
            gram_mma(af, bf, acc);      // acc[r] = G[r0 + (r & 3) + 8 (r >> 2) + 4 half][c0 + 32 wave + l31]
        }
    }
    const int c = c0 + wave * 32 + l31;
    if (c >= C) return;
    float* o = part + (size_t)blockIdx.z * n_rows * C;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = r0 - row0 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (row < n_rows) o[(size_t)row * C + c] = acc[r];
    }
}

// the same partial on the vector unit, one output per thread, p ascending.  grid (ceil(C / 256), n_rows, n * splits)
template <typename T>
__global__ __launch_bounds__(256) void gram_vec_kernel(const T* __restrict__ X, int P, int C, int row0, int n_rows, int splits,
                                                       float* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int img = blockIdx.z / splits, z = blockIdx.z - img * splits;
    const int pb = z * GRAM_PCHUNK, pe = (P - pb < GRAM_PCHUNK) ? P : pb + GRAM_PCHUNK;
    const T* Xi = X + (size_t)img * P * C;
    const int r = row0 + blockIdx.y;
    float acc = 0.f;
    for (int p = pb; p < pe; ++p) acc = fmaf((float)Xi[(size_t)p * C + r], (float)Xi[(size_t)p * C + c], acc);
    part[((size_t)blockIdx.z * n_rows + blockIdx.y) * C + c] = acc;
}

// out[img][e] = the splits' partials of element e, added in ascending p order.  total = n * n_rows * C
__global__ __launch_bounds__(256) void gram_fold_kernel(const float* __restrict__ part, int per_img, int splits, size_t total,
                                                        float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t img = i / per_img, e = i - img * per_img;
        const float* o = part + img * splits * per_img + e;
        float acc = o[0];
        for (int z = 1; z < splits; ++z) acc += o[(size_t)z * per_img];
        out[i] = acc;
    }
}

// stats[img] = (sum of squares, min, max, 0) of the image's per_img outputs: f64 per thread over its elements in ascending order, the
// threads of a wave by shuffles, the waves in a fixed order.  grid (n)
__global__ __launch_bounds__(256) void gram_stats_kernel(const float* __restrict__ out, int per_img, float* __restrict__ stats) {
    __shared__ double rs[4];
    __shared__ float rmn[4], rmx[4];
    const float* o = out + (size_t)blockIdx.x * per_img;
    double ss = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int e = threadIdx.x; e < per_img; e += 256) {
        const float f = o[e];
        ss += (double)f * (double)f;
        mn = fminf(mn, f);
        mx = fmaxf(mx, f);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ss += __shfl_xor(ss, off);
        mn = fminf(mn, __shfl_xor(mn, off));
        mx = fmaxf(mx, __shfl_xor(mx, off));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { rs[wave] = ss; rmn[wave] = mn; rmx[wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* st = stats + (size_t)blockIdx.x * 4;
        st[0] = (float)((rs[0] + rs[1]) + (rs[2] + rs[3]));
        st[1] = fminf(fminf(rmn[0], rmn[1]), fminf(rmn[2], rmn[3]));
        st[2] = fmaxf(fmaxf(rmx[0], rmx[1]), fmaxf(rmx[2], rmx[3]));
        st[3] = 0.f;
    }
}

inline int gram_splits(int P) { return (P + GRAM_PCHUNK - 1) / GRAM_PCHUNK; }

// bytes of partials, 0 for a call that is not served
size_t gram_scratch(int n, int P, int C, int row0, int n_rows, int dtype) {
    if (dtype != DSIM_F32 && dtype != DSIM_BF16 && dtype != DSIM_F16) return 0;
    if (n < 1 || P < 1 || C < 8 || C % 8 || row0 < 0 || n_rows < 1 || n_rows > C - row0) return 0;
    if (n_rows > 65535 || (long)n * gram_splits(P) > 65535) return 0;             // grid axes
    if ((long)n_rows * C > (1l << 30) || (size_t)n * n_rows * C >= (1ull << 40)) return 0;
    return up256((size_t)n * gram_splits(P) * n_rows * C * sizeof(float));
}

int launch_gram_rows(const void* feat, int n, int P, int C, int row0, int n_rows, int dtype, float* out, float* stats, float* part,
                     hipStream_t s) {
    const int splits = gram_splits(P);
    const bool mfma = dtype != DSIM_F32 && n_rows >= 8 && row0 % 8 == 0;
    CK(by_dtype(dtype, [&](auto e) -> int {
        typedef typename decltype(e)::type T;
        if constexpr (sizeof(T) == 2) {
            if (mfma) {
                hipLaunchKernelGGL(gram_mfma_kernel<T>, dim3((C + GC - 1) / GC, (n_rows + GR - 1) / GR, n * splits), dim3(256), 0, s,
                                   (const T*)feat, P, C, row0, n_rows, splits, part);
                DSIM_HIP_CHECK(hipGetLastError());
                return DSIM_OK;
            }
        }
        hipLaunchKernelGGL(gram_vec_kernel<T>, dim3((C + 255) / 256, n_rows, n * splits), dim3(256), 0, s, (const T*)feat, P, C, row0, n_rows,
                           splits, part);
        DSIM_HIP_CHECK(hipGetLastError());
        return DSIM_OK;
    }));
    const size_t total = (size_t)n * n_rows * C;
    hipLaunchKernelGGL(gram_fold_kernel, dim3(ew_blocks(total)), dim3(256), 0, s, (const float*)part, n_rows * C, splits, total, out);
    hipLaunchKernelGGL(gram_stats_kernel, dim3(n), dim3(256), 0, s, (const float*)out, n_rows * C, stats);
    DSIM_HIP_CHECK(hipGetLastError());
    return DSIM_OK;
}

}  // namespace

extern "C" {

int dsim_vgg_create(const dsim_vgg_cfg* cfg, dsim_vgg** out) {
    if (!cfg || !out) return DSIM_ERR_INVALID;
    if (cfg->in_channels < 1 || cfg->in_channels > 4) return DSIM_ERR_INVALID;        // the first-layer kernel's instantiations
    // a conv first and last, a pool only behind a conv, channels in 16-byte segments, a terminator inside the array
    int np = 0;
    while (np < DSIM_VGG_MAX_PLAN && cfg->plan[np] != -1) ++np;
    if (np < 1 || np == DSIM_VGG_MAX_PLAN || cfg->plan[0] <= 0 || cfg->plan[np - 1] <= 0) return DSIM_ERR_INVALID;
    for (int i = 0; i < np; ++i) {
        const int e = cfg->plan[i];
        if (e < 0 || (e > 0 && e % 8) || (e == 0 && cfg->plan[i - 1] == 0)) return DSIM_ERR_INVALID;
    }
    const int st = handle_create(cfg, out);
    if (st == DSIM_OK) (*out)->n_plan = np;
    return st;
}

void dsim_vgg_destroy(dsim_vgg* h) { delete h; }

int dsim_vgg_load_weight(dsim_vgg* h, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim) {
    return handle_load(h, key, dev_ptr, dtype, shape, ndim);
}

int dsim_vgg_finalize(dsim_vgg* h, void* stream) {
    if (!h) return DSIM_ERR_INVALID;
    if (h->finalized) return DSIM_ERR_STATE;
    hipStream_t s = (hipStream_t)stream;
    CK(pack_all(h, s));
    DSIM_HIP_CHECK(hipStreamSynchronize(s));
    h->raw.clear();
    h->finalized = true;
    // every parameter present and of the plan's shape, every conv a shape the GEMM serves: dry walk at the smallest image the pools allow
    int side = 1;
    for (int i = 0; i < h->n_plan; ++i)
        if (h->cfg.plan[i] == 0) side *= 2;
    size_t peak;
    const int st = vgg_plan(h, 1, side, side, &peak, nullptr, nullptr, nullptr);
    if (st != DSIM_OK) { h->finalized = false; return st; }
    return DSIM_OK;
}

int dsim_vgg_profile(dsim_vgg* h, int enable) { return prof_enable(h, enable); }
int dsim_vgg_profile_count(const dsim_vgg* h) { return prof_count(h); }
int dsim_vgg_profile_get(dsim_vgg* h, int i, char* name, int name_cap, double* flops, double* bytes, double* ms) {
    return prof_get(h, i, name, name_cap, flops, bytes, ms);
}

int dsim_vgg_out_shape(const dsim_vgg* hc, int H, int W, int* out_h, int* out_w, int* out_c) {
    dsim_vgg* h = const_cast<dsim_vgg*>(hc);
    if (!h || !out_h || !out_w || !out_c) return DSIM_ERR_INVALID;
    if (!h->finalized) return DSIM_ERR_STATE;
    size_t peak;
    return vgg_plan(h, 1, H, W, &peak, out_h, out_w, out_c);
}

size_t dsim_vgg_workspace_bytes(const dsim_vgg* hc, int n_images, int H, int W) {
    dsim_vgg* h = const_cast<dsim_vgg*>(hc);
    if (!h || !h->finalized) return 0;
    size_t peak;
    if (vgg_plan(h, n_images, H, W, &peak, nullptr, nullptr, nullptr) != DSIM_OK) return 0;
    return peak + 256;
}

int dsim_vgg_features(dsim_vgg* h, const float* pixels, int n_images, int H, int W, void* out, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (!h || !pixels || !out || !workspace || n_images < 1) return DSIM_ERR_INVALID;
    if (!h->finalized) return DSIM_ERR_STATE;
    return run_in_workspace(
        workspace, workspace_bytes, [&](size_t* peak) { return vgg_plan(h, n_images, H, W, peak, nullptr, nullptr, nullptr); },
        [&](Arena& ar) {
            VggWalk w{h, &ar, (hipStream_t)stream, n_images, true};
            return w.go(pixels, H, W, out);
        });
}

int dsim_op_relu(void* x, size_t n_elems, int dtype, void* stream) {
    if (!x || n_elems < 1 || (dtype != DSIM_F32 && dtype != DSIM_BF16 && dtype != DSIM_F16)) return DSIM_ERR_INVALID;
    if (n_elems % (V16 / dtype_size(dtype)) || ((uintptr_t)x & 15)) return DSIM_ERR_INVALID;
    return launch_relu(x, n_elems, dtype, (hipStream_t)stream);
}

int dsim_op_relu_pool2(const void* in, void* out, int n, int H, int W, int C, int dtype, void* stream) {
    if (!in || !out || n < 1 || H < 2 || W < 2 || C < 8 || C % 8) return DSIM_ERR_INVALID;
    if ((dtype != DSIM_F32 && dtype != DSIM_BF16 && dtype != DSIM_F16) || (((uintptr_t)in | (uintptr_t)out) & 15)) return DSIM_ERR_INVALID;
    return launch_relu_pool2(in, out, n, H, W, C, dtype, (hipStream_t)stream);
}

size_t dsim_gram_rows_workspace_bytes(int n, int P, int C, int row0, int n_rows, int dtype) {
    const size_t b = gram_scratch(n, P, C, row0, n_rows, dtype);
    return b ? b + 256 : 0;
}

int dsim_gram_rows(const void* feat, int n, int P, int C, int row0, int n_rows, int dtype, float* out, float* stats, void* workspace,
                   size_t workspace_bytes, void* stream) {
    if (!feat || !out || !stats || !workspace || ((uintptr_t)feat & 15)) return DSIM_ERR_INVALID;
    const size_t need = gram_scratch(n, P, C, row0, n_rows, dtype);
    if (need == 0) return DSIM_ERR_INVALID;
    if (!align_workspace(workspace, workspace_bytes) || workspace_bytes < need) return DSIM_ERR_WORKSPACE;
    return launch_gram_rows(feat, n, P, C, row0, n_rows, dtype, out, stats, (float*)workspace, (hipStream_t)stream);
}

}  // extern "C"
