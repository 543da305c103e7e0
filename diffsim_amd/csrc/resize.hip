// PIL's two-pass 8-bit resample (Pillow Resample.c, ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc) for packed RGB
// uint8 over a ragged batch: the images of a call have their own source sizes and one output size.  It replaces the
// `image.resize(..., LANCZOS)` of process_image (diffsim/diffsim.py:27-33) and the image processors' bicubic
// resize + centre crop of the ViT metrics.  Integer arithmetic only, in PIL's order, so the bytes are PIL's:
//     out = clamp((2^21 + sum_i p[min + i] * k[i]) >> 22, 0, 255)          (int32, arithmetic shift)
// with (min, n) and the 22-bit fixed-point k[] read from tables the caller built (diffsim_amd/resize.py: coeff_table).
//
// resize_h_kernel, one workgroup of 256 threads = (image, RH consecutive source rows of [y_first, y_first + rows), TX = 64 output
//   columns of the crop window):
//     reads   per row, the source bytes [3 min(x0), 3 (min(x1) + n(x1))) of the tile's first and last column, once, as aligned
//             dwords into LDS (the row's last, partial dword byte by byte, so no byte beyond the image is touched); the tile's
//             (min, n) pairs and coefficient rows from the table (shared by the RH rows, served by the caches)
//     writes  temp[row][3 (x - ox) ...] u8, staged in LDS and stored as whole dwords: a temp row is padded to 16 bytes, so a
//             tile's 192 bytes start dword-aligned and a row's last dword may spill into its own padding
//   Workgroups of an image that skips the pass (source width = output width), or past its rows, exit at once.
// resize_v_kernel, one thread = 4 consecutive bytes of one output row of the crop window (256 per workgroup, rows and images
//   over the grid):
//     reads   those 4 byte columns of the temp rows [min(y), min(y) + n(y)) as one dword each (straight from the source rows
//             when the horizontal pass was skipped), and row y's coefficients
//     writes  out[image][y - oy][...] 4 bytes as one dword; a row's last 1..3 bytes byte by byte
//   A skipped vertical pass (source height = output height) is the same walk with the one coefficient 2^22: a copy.
// No atomics, 64-bit offsets; an image's bytes come from its own source, tables and temp alone.
#include <vector>

#include "common.h"

namespace dsim {
namespace {

constexpr int RESIZE_TX = 64;            // output columns per horizontal workgroup
constexpr int RESIZE_LDS = 60 * 1024;    // LDS a horizontal workgroup may take
constexpr int RESIZE_ROWS_MAX = 8;       // source rows per horizontal workgroup, at most

struct ResizeImg {                       // one image, resolved on the host (table ids -> offsets into the table buffer)
    long long src_off, tmp_off;          // bytes into the source buffer / the temp area
    int w, h;
    int hk_off, hk_size;                 // horizontal table: int32 index of its (min, n) rows, ksize; hk_off < 0: pass skipped
    int vk_off, vk_size;                 // vertical table, the same
    int y_first, rows;                   // the source rows the vertical pass reads
    int pad0, pad1;
};
static_assert(sizeof(ResizeImg) == 56, "ResizeImg is copied to the device as bytes");

// The shift and the clamp are kept apart by an opaque copy: written as one expression, hipcc folds two of them into a
// v_ashr_pk_u8_i32 and ORs its result as if the upper 16 bits of the destination were zero; on the MI355X they kept the register's
// previous contents, which came out as stray bits in the two other bytes of the stored dword.
__device__ __forceinline__ int clip8(int acc) {
    int v = acc >> 22;
    asm volatile("" : "+v"(v));
    return min(max(v, 0), 255);
}

__device__ __forceinline__ unsigned load_u32(const unsigned char* p) {       // any alignment
    unsigned v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

__global__ __launch_bounds__(256) void resize_h_kernel(const unsigned char* __restrict__ src, const ResizeImg* __restrict__ imgs,
                                                       const int* __restrict__ tables, unsigned char* __restrict__ temp, int out_w,
                                                       int ox, int cw, int tstride, int RH, int seg_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const ResizeImg im = imgs[blockIdx.z];
    const int r0 = blockIdx.y * RH;
    if (im.hk_off < 0 || r0 >= im.rows) return;
    const int nr = min(RH, im.rows - r0);
    const int j0 = blockIdx.x * RESIZE_TX, nx = min(RESIZE_TX, cw - j0);
    const int* bounds = tables + im.hk_off;
    const int* coef = bounds + 2 * (size_t)out_w;
    // the tile's source window; the clamps hold whatever the table says
    const int xl = ox + j0 + nx - 1;
    const int xs = min(max(bounds[2 * (ox + j0)], 0), im.w);
    int xe = min(max(bounds[2 * xl] + bounds[2 * xl + 1], xs), im.w);
    xe = min(xe, xs + (seg_stride - 8) / 3);
    unsigned char* stage = lds + (size_t)RH * seg_stride;                        // [RH][192] output bytes
    const size_t img_end = (size_t)im.src_off + (size_t)3 * im.w * im.h;
    for (int r = 0; r < nr; ++r) {
        const size_t a = (size_t)im.src_off + ((size_t)(im.y_first + r0 + r) * im.w + xs) * 3;
        const size_t a0 = a & ~(size_t)3;
        const int nd = (int)((a + (size_t)(xe - xs) * 3 - a0 + 3) >> 2);
        unsigned* row = (unsigned*)(lds + (size_t)r * seg_stride);
        for (int i = threadIdx.x; i < nd; i += 256) {
            const size_t g = a0 + (size_t)i * 4;
            unsigned v;
            if (g + 4 <= img_end) {
                v = *(const unsigned*)(src + g);
            } else {
                v = 0;
                for (int b = 0; b < 4; ++b)
                    if (g + b < img_end) v |= (unsigned)src[g + b] << (8 * b);
            }
            row[i] = v;
        }
    }
    __syncthreads();
    for (int it = threadIdx.x; it < nr * nx; it += 256) {
        const int r = it / nx, j = it - r * nx;
        const int x = ox + j0 + j;
        const int xmin = min(max(bounds[2 * x], xs), xe);
        const int n = min(min(bounds[2 * x + 1], im.hk_size), xe - xmin);
        const int* k = coef + (size_t)x * im.hk_size;
        const size_t a = (size_t)im.src_off + ((size_t)(im.y_first + r0 + r) * im.w + xs) * 3;
        const unsigned char* p = lds + (size_t)r * seg_stride + (a & 3) + (size_t)(xmin - xs) * 3;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int i = 0; i < n; ++i) {
            const int kv = k[i];
            a0 += p[3 * i] * kv;
            a1 += p[3 * i + 1] * kv;
            a2 += p[3 * i + 2] * kv;
        }
        unsigned char* o = stage + r * (RESIZE_TX * 3) + j * 3;
        o[0] = (unsigned char)clip8(a0);
        o[1] = (unsigned char)clip8(a1);
        o[2] = (unsigned char)clip8(a2);
    }
    __syncthreads();
    const int ndw = (nx * 3 + 3) >> 2;                                           // <= 48; the last one may reach into the row's padding
    for (int it = threadIdx.x; it < nr * ndw; it += 256) {
        const int r = it / ndw, d = it - r * ndw;
        unsigned* dst = (unsigned*)(temp + im.tmp_off + (size_t)(r0 + r) * tstride + (size_t)j0 * 3);
        dst[d] = ((const unsigned*)(stage + r * (RESIZE_TX * 3)))[d];
    }
}

__global__ __launch_bounds__(256) void resize_v_kernel(const unsigned char* __restrict__ src, const ResizeImg* __restrict__ imgs,
                                                       const int* __restrict__ tables, const unsigned char* __restrict__ temp,
                                                       unsigned char* __restrict__ out, int out_h, int ox, int oy, int cw, int ch,
                                                       int tstride) {
    const ResizeImg im = imgs[blockIdx.z];
    const int rowb = cw * 3, groups = (rowb + 3) >> 2;
    const int it = blockIdx.x * 256 + threadIdx.x;
    if (it >= groups * ch) return;
    const int yj = it / groups, b = (it - yj * groups) * 4;
    const int y = oy + yj;
    // the rows this pass walks: the temp the horizontal pass wrote (row 0 = source row y_first), or the source itself
    const unsigned char* base;
    size_t stride;
    if (im.hk_off >= 0) {
        base = temp + im.tmp_off;
        stride = (size_t)tstride;
    } else {
        base = src + im.src_off + ((size_t)im.y_first * im.w + ox) * 3;
        stride = (size_t)im.w * 3;
    }
    int ymin, n;
    const int* k = nullptr;
    if (im.vk_off >= 0) {
        const int* bounds = tables + im.vk_off;
        ymin = min(max(bounds[2 * y] - im.y_first, 0), im.rows);
        n = min(min(bounds[2 * y + 1], im.vk_size), im.rows - ymin);
        k = bounds + 2 * (size_t)out_h + (size_t)y * im.vk_size;
    } else {                                                                     // height unchanged: row y itself, weight 1.0
        ymin = min(y - im.y_first, im.rows - 1);
        n = 1;
    }
    const unsigned char* p = base + (size_t)ymin * stride + b;
    unsigned char* o = out + ((size_t)blockIdx.z * ch + yj) * rowb + b;
    if (b + 4 <= rowb) {
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
        for (int i = 0; i < n; ++i) {
            const int kv = k ? k[i] : (1 << 22);
            const unsigned v = load_u32(p + (size_t)i * stride);
            a0 += (int)(v & 255u) * kv;
            a1 += (int)((v >> 8) & 255u) * kv;
            a2 += (int)((v >> 16) & 255u) * kv;
            a3 += (int)(v >> 24) * kv;
        }
        const unsigned v = (unsigned)clip8(a0) | (unsigned)clip8(a1) << 8 | (unsigned)clip8(a2) << 16 | (unsigned)clip8(a3) << 24;
        __builtin_memcpy(o, &v, 4);
    } else {                                                                     // the row's last 1..3 bytes
        for (int c = 0; c < rowb - b; ++c) {
            int a = 1 << 21;
            for (int i = 0; i < n; ++i) a += (int)p[(size_t)i * stride + c] * (k ? k[i] : (1 << 22));
            o[c] = (unsigned char)clip8(a);
        }
    }
}

inline size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int temp_stride(int cw) { return (int)up((size_t)cw * 3, 16); }

// Every refusal of dsim_resize_u8 that needs no device, and the sizes a launch uses.  Returns DSIM_OK or DSIM_ERR_INVALID.
struct ResizePlan {
    size_t desc_bytes, temp_bytes;
    int any_h, max_rows, RH, seg_stride;
};

int resize_plan(const dsim_resize_image* images, int n, const dsim_resize_table* tables, int n_tables, size_t table_ints, int out_w,
                int out_h, int ox, int oy, int cw, int ch, size_t src_bytes, ResizePlan* plan) {
    if (!images || !tables || n < 1 || n > 65535 || n_tables < 1 || out_w < 1 || out_h < 1 || cw < 1 || ch < 1 || ox < 0 || oy < 0)
        return DSIM_ERR_INVALID;
    if ((long long)ox + cw > out_w || (long long)oy + ch > out_h || out_w > (1 << 20) || out_h > (1 << 20)) return DSIM_ERR_INVALID;
    for (int t = 0; t < n_tables; ++t) {
        const dsim_resize_table& tb = tables[t];
        if (tb.ksize < 1 || tb.in_size < 1 || tb.out_size < 1 || tb.offset < 0) return DSIM_ERR_INVALID;
        const size_t ints = (size_t)tb.out_size * (2 + (size_t)tb.ksize);
        if ((size_t)tb.offset > table_ints || ints > table_ints - (size_t)tb.offset || table_ints >= ((size_t)1 << 31))
            return DSIM_ERR_INVALID;
    }
    const size_t tstride = (size_t)temp_stride(cw);
    size_t temp = 0, seg_px = 0;
    int any_h = 0, max_rows = 0;
    for (int i = 0; i < n; ++i) {
        const dsim_resize_image& im = images[i];
        if (im.w < 1 || im.h < 1 || im.w > (1 << 20) || im.h > (1 << 20) || im.src_offset < 0 || (im.src_offset & 15)) return DSIM_ERR_INVALID;
        const size_t bytes = (size_t)3 * im.w * im.h;
        if ((size_t)im.src_offset > src_bytes || bytes > src_bytes - (size_t)im.src_offset) return DSIM_ERR_INVALID;
        if (im.h_table < -1 || im.h_table >= n_tables || im.v_table < -1 || im.v_table >= n_tables) return DSIM_ERR_INVALID;
        if (im.h_table < 0 ? im.w != out_w : (tables[im.h_table].in_size != im.w || tables[im.h_table].out_size != out_w))
            return DSIM_ERR_INVALID;
        if (im.v_table < 0 ? im.h != out_h : (tables[im.v_table].in_size != im.h || tables[im.v_table].out_size != out_h))
            return DSIM_ERR_INVALID;
        if (im.y_first < 0 || im.rows < 1 || (long long)im.y_first + im.rows > im.h) return DSIM_ERR_INVALID;
        if (im.v_table < 0 && (im.y_first > oy || im.y_first + im.rows < oy + ch)) return DSIM_ERR_INVALID;
        if (im.h_table >= 0) {
            if (im.temp_offset < 0 || (im.temp_offset & 15)) return DSIM_ERR_INVALID;
            temp = temp > (size_t)im.temp_offset + (size_t)im.rows * tstride ? temp : (size_t)im.temp_offset + (size_t)im.rows * tstride;
            any_h = 1;
            max_rows = max_rows > im.rows ? max_rows : im.rows;
            // source pixels under one tile of TX columns: the windows' starts move by at most (TX - 1) scale + 1, a window is <= ksize
            const dsim_resize_table& tb = tables[im.h_table];
            size_t px = ((size_t)(RESIZE_TX - 1) * tb.in_size + tb.out_size - 1) / tb.out_size + (size_t)tb.ksize + 2;
            px = px < (size_t)im.w ? px : (size_t)im.w;
            seg_px = seg_px > px ? seg_px : px;
        }
    }
    plan->desc_bytes = up((size_t)n * sizeof(ResizeImg), 256);
    plan->temp_bytes = up(temp, 256);
    plan->any_h = any_h;
    plan->max_rows = max_rows;
    plan->seg_stride = (int)up(seg_px * 3 + 8, 16);
    const size_t per_row = (size_t)plan->seg_stride + RESIZE_TX * 3;
    if (any_h && per_row > (size_t)RESIZE_LDS) return DSIM_ERR_INVALID;          // more than ~300 source pixels per output pixel
    int RH = any_h ? (int)((size_t)RESIZE_LDS / per_row) : 1;
    plan->RH = RH > RESIZE_ROWS_MAX ? RESIZE_ROWS_MAX : RH;
    if ((max_rows + plan->RH - 1) / plan->RH > 65535) return DSIM_ERR_INVALID;
    if ((size_t)ch * ((size_t)cw * 3 / 4 + 1) >= ((size_t)1 << 31)) return DSIM_ERR_INVALID;
    return DSIM_OK;
}

}  // namespace
}  // namespace dsim

using namespace dsim;

extern "C" size_t dsim_resize_u8_workspace_bytes(const dsim_resize_image* images, int n, const dsim_resize_table* tables, int n_tables,
                                                 size_t table_ints, int out_w, int out_h, int ox, int oy, int cw, int ch,
                                                 size_t src_bytes) {
    ResizePlan p;
    if (resize_plan(images, n, tables, n_tables, table_ints, out_w, out_h, ox, oy, cw, ch, src_bytes, &p) != DSIM_OK) return 0;
    return p.desc_bytes + p.temp_bytes;
}

extern "C" int dsim_resize_u8(const unsigned char* src, size_t src_bytes, const dsim_resize_image* images, int n,
                              const int32_t* table_data, size_t table_ints, const dsim_resize_table* tables, int n_tables, int out_w,
                              int out_h, int ox, int oy, int cw, int ch, unsigned char* out, void* workspace, size_t workspace_bytes,
                              void* stream) {
    if (!src || !table_data || !out || !workspace) return DSIM_ERR_INVALID;
    ResizePlan p;
    const int rc = resize_plan(images, n, tables, n_tables, table_ints, out_w, out_h, ox, oy, cw, ch, src_bytes, &p);
    if (rc != DSIM_OK) return rc;
    if (workspace_bytes < p.desc_bytes + p.temp_bytes) return DSIM_ERR_WORKSPACE;
    if (((size_t)workspace & 15) || ((size_t)src & 15)) return DSIM_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    std::vector<ResizeImg> host((size_t)n);
    for (int i = 0; i < n; ++i) {
        const dsim_resize_image& im = images[i];
        ResizeImg& d = host[(size_t)i];
        d.src_off = im.src_offset;
        d.tmp_off = im.h_table >= 0 ? im.temp_offset : 0;
        d.w = im.w;
        d.h = im.h;
        d.hk_off = im.h_table >= 0 ? (int)tables[im.h_table].offset : -1;
        d.hk_size = im.h_table >= 0 ? tables[im.h_table].ksize : 1;
        d.vk_off = im.v_table >= 0 ? (int)tables[im.v_table].offset : -1;
        d.vk_size = im.v_table >= 0 ? tables[im.v_table].ksize : 1;
        d.y_first = im.y_first;
        d.rows = im.rows;
        d.pad0 = d.pad1 = 0;
    }
    ResizeImg* dimg = (ResizeImg*)workspace;
    unsigned char* temp = (unsigned char*)workspace + p.desc_bytes;
    // pageable host memory: the copy has left `host` when the call returns
    DSIM_HIP_CHECK(hipMemcpyAsync(dimg, host.data(), (size_t)n * sizeof(ResizeImg), hipMemcpyHostToDevice, s));
    const int tstride = temp_stride(cw);
    if (p.any_h) {
        const size_t lds = (size_t)p.RH * ((size_t)p.seg_stride + RESIZE_TX * 3);
        const dim3 grid((unsigned)((cw + RESIZE_TX - 1) / RESIZE_TX), (unsigned)((p.max_rows + p.RH - 1) / p.RH), (unsigned)n);
        hipLaunchKernelGGL(resize_h_kernel, grid, dim3(256), lds, s, src, dimg, table_data, temp, out_w, ox, cw, tstride, p.RH,
                           p.seg_stride);
        DSIM_HIP_CHECK(hipGetLastError());
    }
    const size_t items = (size_t)ch * (((size_t)cw * 3 + 3) / 4);
    hipLaunchKernelGGL(resize_v_kernel, dim3((unsigned)((items + 255) / 256), 1, (unsigned)n), dim3(256), 0, s, src, dimg, table_data,
                       temp, out, out_h, ox, oy, cw, ch, tstride);
    DSIM_HIP_CHECK(hipGetLastError());
    return DSIM_OK;
}
