// Text attention maps and text-guided regions: which image tokens listen to which prompt tokens.  The reference declares
// `--use_text_attn`, "use the cross-attention results of text to guide conditional similarity" (argprocess.py:17), and implements
// nothing behind it; these kernels compute the tapped block's own cross-attention (attn2) for its own sake and turn it into a token
// region per image, which the region tail (regions.hip) then scores.  They share the tiled core's fragments, MFMA wrappers, K row
// geometry, head-dim dispatch and un-rescaled logit routine (attn_core.h) with align.hip; there is no V and no O.
#include "attn_core.h"

namespace dsim {
namespace {

constexpr int TA_KEYS = 128;     // the most prompt tokens a call takes: four 32-key blocks, all resident in LDS and in registers
constexpr int TA_NB = TA_KEYS / 32;

// For image i, on the conditional CFG half alone (batch element e = 2 i + 1; its context row is 1 of a shared [uncond, cond] pair,
// e of a per-element table):
//   P_h[n][l] = softmax_l(xq_h[n,:] . xk_h[l,:] / sqrt(D)),   T[n][l] = mean over the H heads of P_h[n][l]   (heads ascending)
//   saliency[n] = sum_l w[l] T[n][l]                                                                         (f32 fma, l ascending)
// The logits come from the stored values (align_logits: accumulators from 0, no pre-scaled query); the scale enters in f32,
// e = exp2(fma(s, c, -m c)) with c = log2(e) / sqrt(D), and nothing is rounded to 16 bits on the way to T: align.hip's arithmetic.
// L <= 128, so a row's whole key set is in registers and the softmax is one pass: no running maximum, no rescale.
//
// grid (ceil(N / 128), n_images); four waves x 32 query rows.  Per head: K_h (L rows x D, the rows beyond L and the padding columns
// keep the zeros of the one fill) into LDS, the logits of ceil(L / 32) blocks, keys >= L to -inf, the row maximum and denominator
// in-lane plus one permlane32_swap each, acc = fma(e, 1 / l, acc).  Every output element has one writer; status is a plain store of
// 1 by any row that saw a non-finite probability, into a word the launcher zeroed.  Nothing depends on the other images of the
// launch.
template <typename T, int D>
__global__ __launch_bounds__(256) void text_attn_kernel(const T* __restrict__ xq, int ldq, const T* __restrict__ xk, int ldk, int n_kv,
                                                         int H, int N, int L, float c, float rh, const float* __restrict__ weight,
                                                         int n_w, float* __restrict__ attn, float* __restrict__ saliency,
                                                         int32_t* __restrict__ status) {
    typedef ACfg<T, D> C;
    constexpr int CPRD = D / C::VEC;             // real 16-B chunks per K row
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int img = blockIdx.y, e = 2 * img + 1;
    const int q = blockIdx.x * 128 + wave * 32 + l31, qc = q < N ? q : N - 1;
    const T* qrow = xq + ((size_t)e * N + qc) * ldq;
    const T* kimg = xk + (size_t)(n_kv == 2 ? 1 : e) * L * ldk;
    const int nb = (L + 31) / 32;
    {
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (int o = tid * 16; o < TA_KEYS * C::RS; o += 256 * 16) *reinterpret_cast<u32x4*>(lds + o) = z;
    }
    f32x16 acc[TA_NB];
#pragma unroll
    for (int jb = 0; jb < TA_NB; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[jb][r] = 0.f;
    for (int h = 0; h < H; ++h) {
        QFrags<T, D> qf;
        align_load_q<T, D>(qf, qrow + h * D, half);
        __syncthreads();                   // the fill is done / the previous head's fragments are read
        for (int idx = tid; idx < L * CPRD; idx += 256) {
            const int r = idx / CPRD, ch = idx - r * CPRD;
            *reinterpret_cast<u32x4*>(lds + r * C::RS + ch * 16) =
                *reinterpret_cast<const u32x4*>(kimg + (size_t)r * ldk + h * D + ch * C::VEC);
        }
        __syncthreads();
        f32x16 s[TA_NB];
        float tmax = -INFINITY;
#pragma unroll
        for (int jb = 0; jb < TA_NB; ++jb) {
            if (jb < nb) {
                s[jb] = align_logits<T, D>(qf, lds, jb, l31, half);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (align_key(jb, r, half) >= L) s[jb][r] = -INFINITY;
                    tmax = fmaxf(tmax, s[jb][r]);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[jb][r] = -INFINITY;
            }
        }
        tmax = max_halves(tmax);
        const float mc = -tmax * c;
        float l = 0.f;
#pragma unroll
        for (int jb = 0; jb < TA_NB; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[jb][r] = __builtin_amdgcn_exp2f(fmaf(s[jb][r], c, mc));
                l += s[jb][r];
            }
        l = half_sum(l);
        const float inv = 1.0f / l;
#pragma unroll
        for (int jb = 0; jb < TA_NB; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[jb][r] = fmaf(s[jb][r], inv, acc[jb][r]);
    }
    // the mean over the heads; this half's keys < L: the non-finite test and the attention row
    bool bad = false;
    float* arow = attn ? attn + ((size_t)img * N + qc) * L : nullptr;
#pragma unroll
    for (int jb = 0; jb < TA_NB; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = acc[jb][r] * rh;
            acc[jb][r] = v;
            const int key = align_key(jb, r, half);
            if (key < L) {
                bad = bad || !(v - v == 0.0f);
                if (attn && q < N) arow[key] = v;
            }
        }
    if (status && bad && q < N) status[img] = 1;
    if (saliency) {
        // keys ascending: the lower half holds keys 8 g .. 8 g + 3 of a block's group g, the upper half 8 g + 4 .. 8 g + 7; both
        // lanes of a row run the same chain on the swapped values, the lower one stores
        const float* w = weight + (size_t)(n_w == 1 ? 0 : img) * L;
        float sv = 0.f;
#pragma unroll
        for (int jb = 0; jb < TA_NB; ++jb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float lo[4], hi[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned u = __float_as_uint(acc[jb][4 * g + j]);
                    const auto p = __builtin_amdgcn_permlane32_swap(u, u, false, false);
                    lo[j] = __uint_as_float(p[0]);
                    hi[j] = __uint_as_float(p[1]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int key = jb * 32 + 8 * g + j;
                    if (key < L) sv = fmaf(w[key], lo[j], sv);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int key = jb * 32 + 8 * g + 4 + j;
                    if (key < L) sv = fmaf(w[key], hi[j], sv);
                }
            }
        if (half == 0 && q < N) saliency[(size_t)img * N + q] = sv;
    }
}

// One workgroup per image: m = the mean saliency, summed in f64 (each thread its tokens t = tid, tid + 256, ... ascending, then a
// fixed tree over the 256 partial sums: the order depends on N alone); token n is on iff (double)s[n] >= (double)rel_threshold * m;
// if no token passes -- a threshold above every token, or non-finite saliency -- every token is on (regions.token_mask's fallback,
// foreground_feature_averaging.py:70-71 of the reference).  Mask bytes [N], the count.
__global__ __launch_bounds__(256) void text_region_kernel(const float* __restrict__ saliency, int N, float rel_threshold,
                                                          uint8_t* __restrict__ mask, int32_t* __restrict__ counts) {
    __shared__ double red[256];
    __shared__ int cnt[256];
    const int tid = threadIdx.x, img = blockIdx.x;
    const float* s = saliency + (size_t)img * N;
    double a = 0.0;
    for (int t = tid; t < N; t += 256) a += (double)s[t];
    red[tid] = a;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    const double lim = (double)rel_threshold * (red[0] / (double)N);
    int n = 0;
    for (int t = tid; t < N; t += 256) n += (double)s[t] >= lim ? 1 : 0;
    cnt[tid] = n;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) cnt[tid] += cnt[tid + st];
        __syncthreads();
    }
    const int on = cnt[0];
    if (mask)
        for (int t = tid; t < N; t += 256) mask[(size_t)img * N + t] = (on == 0 || (double)s[t] >= lim) ? 1 : 0;
    if (counts && tid == 0) counts[img] = on == 0 ? N : on;
}

template <typename T>
int launch_text_attn_t(const void* xq, int ldq, const void* xk, int ldk, int n_images, int n_kv, int H, int N, int L, int D,
                       const float* weight, int n_w, float* attn, float* saliency, int32_t* status, hipStream_t s) {
    return with_head_dim(D, [&](auto dc) -> int {
        constexpr int Dc = decltype(dc)::value;
        // (128 keys x 160 f32 columns pass the 64 KB a kernel has without asking: every instantiation goes through launch_lds)
        return launch_lds<text_attn_kernel<T, Dc>>(dim3((N + 127) / 128, n_images), dim3(256), TA_KEYS * ACfg<T, Dc>::RS, s, (const T*)xq,
                                                   ldq, (const T*)xk, ldk, n_kv, H, N, L, scale_log2_of(Dc), 1.0f / (float)H, weight, n_w,
                                                   attn, saliency, status);
    });
}

}  // namespace

inline namespace DSIM_H16_NS {
// the saliency of a call that asks for regions and not for the saliency itself, [n_images][N] f32; 0 for a shape not served
size_t text_attention_scratch_bytes(int n_images, int N, int L) {
    if (n_images < 1 || n_images > 65535 || N < 1 || L < 1 || L > TA_KEYS) return 0;
    return (size_t)n_images * N * sizeof(float);
}

// text attention maps, saliency and regions (text_attn_kernel, text_region_kernel): any head dim of DSIM_FOR_EACH_D, any N,
// 1 <= L <= 128, the three dtypes.  Every check before the first enqueue.
int launch_text_attention(const void* xq, int ldq, const void* xk, int ldk, int n_images, int n_kv, int H, int N, int L, int D, int dtype,
                          const float* weight, int n_w, float rel_threshold, float* attn, float* saliency, uint8_t* mask, int32_t* counts,
                          int32_t* status, void* scratch, size_t scratch_bytes, hipStream_t s) {
    const size_t need = text_attention_scratch_bytes(n_images, N, L);
    if (need == 0 || H < 1 || !xq || !xk) return DSIM_ERR_INVALID;
    if (dtype != DSIM_F32 && dtype != DSIM_BF16 && dtype != DSIM_F16) return DSIM_ERR_INVALID;
    if (with_head_dim(D, [](auto) { return DSIM_OK; }) != DSIM_OK) return DSIM_ERR_INVALID;
    if (n_kv != 2 && n_kv != 2 * n_images) return DSIM_ERR_INVALID;
    // rows of 16-byte chunks: the leading dimensions in whole chunks, the bases aligned
    const int vec = 16 / (int)dtype_size(dtype);
    if (ldq < H * D || ldk < H * D || ldq % vec || ldk % vec || ((uintptr_t)xq & 15) || ((uintptr_t)xk & 15)) return DSIM_ERR_INVALID;
    if (!(rel_threshold >= 0.0f) || !(rel_threshold - rel_threshold == 0.0f)) return DSIM_ERR_INVALID;
    const bool region = mask || counts;
    if ((saliency || region) && (!weight || (n_w != 1 && n_w != n_images))) return DSIM_ERR_INVALID;
    if (!scratch || scratch_bytes < need) return DSIM_ERR_WORKSPACE;
    return by_h16_dtype(
        dtype,
        [&](auto e) -> int {
            float* sal = saliency ? saliency : (region ? (float*)scratch : nullptr);
            if (status) DSIM_HIP_CHECK(hipMemsetAsync(status, 0, (size_t)n_images * sizeof(int32_t), s));
            const int st = launch_text_attn_t<typename decltype(e)::type>(xq, ldq, xk, ldk, n_images, n_kv, H, N, L, D, weight, n_w, attn, sal,
                                                                          status, s);
            if (st != DSIM_OK) return st;
            if (region) {
                hipLaunchKernelGGL(text_region_kernel, dim3(n_images), dim3(256), 0, s, (const float*)sal, N, rel_threshold, mask, counts);
                DSIM_HIP_CHECK(hipGetLastError());
            }
            return DSIM_OK;
        },
        [&] {
            return DSIM_F16_TWIN(launch_text_attention(xq, ldq, xk, ldk, n_images, n_kv, H, N, L, D, dtype, weight, n_w, rel_threshold, attn,
                                                       saliency, mask, counts, status, scratch, scratch_bytes, s));
        });
}
}  // namespace DSIM_H16_NS

}  // namespace dsim
