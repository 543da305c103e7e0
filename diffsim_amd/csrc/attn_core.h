// The tiled attention core for gfx950: one wave's 32 query rows against any number of keys (attend), with the Q fragments, the
// O^T accumulators and the K / V staging it works on, and the host-side head-dim dispatch.  Shared by exactly six sources: the
// attention kernels (attention.hip), the score tails (tails.hip), the region scores (regions.hip: attend over listed rows), the
// soft region scores (soft_regions.hip: listed rows and a bias per key), the token alignments (align.hip) and the text attention maps
// (textattn.hip) -- the last two take the configuration, fragments, MFMA wrappers, head-dim dispatch and the un-rescaled logit
// routine, not attend; everything here lives in their dsim::(anonymous namespace).
//
// Tiling: a workgroup = 4 waves = 128 query rows of one (batch, head); each wave owns 32 rows and
// sweeps the keys in 64-row tiles shared through LDS.
//   - S^T = K Q^T is computed with K as the MFMA A operand and Q as B ("swapped QK^T"), so a lane
//     holds one query column of S^T in its accumulator registers: the row max is a per-lane
//     reduction over registers plus one exchange between the two lane halves, and the accumulator
//     is directly the B operand of O^T = V^T P^T (no LDS round trip for P).
//   - Q is pre-scaled by log2(e)/sqrt(D) and the S^T accumulators START at -m (the running row
//     max), so P = exp2(acc) needs no subtract and no multiply: per score element the VALU does
//     one v_exp, half a v_max3 and half a v_cvt_pk.  O is rescaled only in tiles where some row's
//     max grew (exact: alpha == 1 for the other rows).
//   - The softmax denominator comes out of the PV MFMAs: when the head dim leaves a spare column
//     in the 32-wide d block (D = 40, 72, 80, 16) the staged V tile carries a column of ones, so
//     row D of O^T accumulates sum(P) and is rescaled together with O.
//   - V^T fragments come from the row-major V tile by ds_read_b64_tr_b16 (h16) / ds_read_b32 (f32).
//   - h16: next tile's global loads are in flight during the current tile's compute (registers
//     -> double-buffered LDS, one barrier per tile).  f32 parity mode: simple single buffer.
// h16 path: v_mfma_f32_32x32x16_bf16; fp32 parity path: v_mfma_f32_32x32x2_f32 (exact f32).
#pragma once
#include "common.h"

#include <type_traits>

namespace dsim {
namespace {

constexpr int KT = 64;   // kv rows per LDS tile

template <typename T, int D> struct ACfg {
    static constexpr int ES = sizeof(T);
    static constexpr int VEC = 16 / ES;
    static constexpr int NKS = (D + 15) / 16;     // 16-deep k steps over d (QK^T)
    static constexpr int NDB = (D + 31) / 32;     // 32-wide output blocks over d (PV)
    static constexpr int DPL = NDB * 32;          // LDS columns (zero padded)
    static constexpr bool ONES = D < DPL;         // spare column -> ones column gives the row sum
    // K tile: only the NKS*16 columns QK^T reads (h16); row stride an odd number of 16-B slots (ds_read_b128)
    static constexpr int DPLK = (ES == 2) ? NKS * 16 : DPL;
    static constexpr int RS = DPLK * ES + 16;
    // h16, D = 8 (mod 16): K carries a ones column at d = D and Q carries -m there, so S^T comes out of the MFMAs
    // already relative to the running max and the accumulators start at the constant 0 (no per-tile register fill).
    // Any per-row reference cancels in the softmax, so -m rounded to h16 is exact as long as m itself is kept rounded.
    static constexpr bool KONE = (ES == 2) && (D % 16 == 8);
    // V tile row stride.  h16: the transposed reads (ds_read_b64_tr_b16) take, per 32-lane half, a
    // 4-row x 32-column block = 4 rows x 16 dwords; they are conflict-free when the row stride is
    // 16 or 48 dwords mod 64 (four rows tile the 64 banks).  f32: plain ds_read_b32, same as K.
    static constexpr int RSV = (ES == 2) ? (((DPL * 2) % 256 == 64 || (DPL * 2) % 256 == 192) ? DPL * 2 : DPL * 2 + 64) : RS;
    static constexpr int CPR = DPL / VEC;         // 16-B chunks per row
    static constexpr int TILEK = KT * RS;
    static constexpr int TILE = (KT * RS + KT * RSV + 1) / 2;   // average, so that 2*TILE = K tile + V tile
    // double-buffered staging, except for the widest heads: there two tile pairs (83 KB) would leave one workgroup per
    // CU; a single pair lets a second workgroup hide this one's load latency instead
    static constexpr bool PIPE = sizeof(T) == 2 && DPL < 160;
    static constexpr int LDS = (PIPE ? 4 : 2) * TILE;
    // waves per SIMD the register budget is held to (occupancy hides the serial MFMA/VALU phases)
    // (4 workgroups per CU need <= 40 KB of LDS each: true for d <= 48 now that the K tile is 48 columns wide)
    static constexpr int WPS = (sizeof(T) == 2 && DPL <= 64) ? (LDS <= 40 * 1024 ? 4 : 3) : ((sizeof(T) == 2 && DPL <= 96) ? 2 : (sizeof(T) == 2 ? 2 : 1));
};

struct FragF32 { f32x4 lo, hi; };
template <typename T> struct FragOf { typedef h16x8 type; };
template <> struct FragOf<float> { typedef FragF32 type; };

__device__ __forceinline__ void zero_frag(h16x8& f) {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (h16)0.0f;
}
__device__ __forceinline__ void zero_frag(FragF32& f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f.lo[i] = f.hi[i] = 0.f;
}
// load 8 consecutive elements and pre-scale them (Q only)
__device__ __forceinline__ void gload_frag_scaled(h16x8& f, const h16* p, float sc) {
    const h16x8 t = *reinterpret_cast<const h16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (h16)((float)t[i] * sc);
}
__device__ __forceinline__ void gload_frag_scaled(FragF32& f, const float* p, float sc) {
    f.lo = *reinterpret_cast<const f32x4*>(p) * sc;
    f.hi = *reinterpret_cast<const f32x4*>(p + 4) * sc;
}
__device__ __forceinline__ void lload_frag(h16x8& f, const char* p) { f = *reinterpret_cast<const h16x8*>(p); }
__device__ __forceinline__ void lload_frag(FragF32& f, const char* p) {
    f.lo = *reinterpret_cast<const f32x4*>(p);
    f.hi = *reinterpret_cast<const f32x4*>(p + 16);
}
__device__ __forceinline__ void mma(const h16x8& a, const h16x8& b, f32x16& c) {
    c = H16_MFMA_32x32x16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ void mma(const FragF32& a, const FragF32& b, f32x16& c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.lo[j], b.lo[j], c, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.hi[j], b.hi[j], c, 0, 0, 0);
}

// Q fragments of this wave's 32 query rows (pre-scaled by log2(e)/sqrt(D)), resident in registers.
template <typename T, int D> struct QFrags { typename FragOf<T>::type f[ACfg<T, D>::NKS]; };
template <typename T, int D> struct OAcc { f32x16 b[ACfg<T, D>::NDB]; };

template <typename T, int D>
__device__ __forceinline__ void load_q(QFrags<T, D>& qf, const T* qrow /*row base + h*D*/, int half, float scale_log2) {
#pragma unroll
    for (int ks = 0; ks < ACfg<T, D>::NKS; ++ks) {
        const int d0 = 16 * ks + 8 * half;
        if (d0 < D) gload_frag_scaled(qf.f[ks], qrow + d0, scale_log2);
        else zero_frag(qf.f[ks]);
    }
}

// Staging of one KT-row tile of K and V, split in a load half and a store half so the global loads can be
// issued a whole tile ahead of the LDS writes.  Only the D real columns move per tile: the zero padding up
// to DPL columns (and, with ONES, the 1.0 in column D of V) is written ONCE per attend() by tile_init.
// Rows >= Nk of a ragged tile are never stored: they keep zeros or stale finite values, and their scores
// are masked to -inf, so they contribute exactly 0.
template <typename T, int D> struct StageRegs {
    static constexpr int CPRD = D / ACfg<T, D>::VEC;                 // real 16-B chunks per row
    static constexpr int N = (KT * CPRD + 255) / 256;
    u32x4 k[N], v[N];
    unsigned goff[N];       // element offset of this thread's chunk inside a tile (row * ldk + col)
    unsigned loff[N];       // byte offset inside the K tile image; the V image uses lvoff
    unsigned lvoff[N];
    int row[N];             // tile row, or KT when this thread has no chunk in round i
};

template <typename T> __device__ __forceinline__ u32x4 one_chunk();
template <> __device__ __forceinline__ u32x4 one_chunk<h16>() { u32x4 r = {DSIM_H16_ONE_BITS, 0u, 0u, 0u}; return r; }   // 1.0 in element 0
template <> __device__ __forceinline__ u32x4 one_chunk<float>() { u32x4 r = {0x3F800000u, 0u, 0u, 0u}; return r; }

template <typename T, int D>
__device__ __forceinline__ void tile_init(StageRegs<T, D>& sr, char* lds, int ldk, int Nk, int tid) {
    typedef ACfg<T, D> C;
    typedef StageRegs<T, D> SR;
    const u32x4 z = {0u, 0u, 0u, 0u};
    // zero fill is needed for the padding columns and for the never-stored rows of a ragged last tile
    if (D < C::DPL || (Nk % KT) != 0)
        for (int o = tid * 16; o < C::LDS; o += 256 * 16) *reinterpret_cast<u32x4*>(lds + o) = z;
#pragma unroll
    for (int i = 0; i < SR::N; ++i) {
        const int idx = tid + i * 256;
        const int r = idx / SR::CPRD, c = idx - r * SR::CPRD;
        sr.row[i] = idx < KT * SR::CPRD ? r : KT;
        sr.goff[i] = (unsigned)r * (unsigned)ldk + (unsigned)c * C::VEC;
        sr.loff[i] = (unsigned)(r * C::RS + c * 16);
        sr.lvoff[i] = (unsigned)(C::TILEK + r * C::RSV + c * 16);
    }
    if constexpr (C::ONES) {
        __syncthreads();
        constexpr int NBUF = C::PIPE ? 2 : 1;
        for (int i = tid; i < KT * NBUF; i += 256) {
            const int buf = i / KT, r = i - buf * KT;
            *reinterpret_cast<u32x4*>(lds + buf * 2 * C::TILE + C::TILEK + r * C::RSV + (D / C::VEC) * 16) = one_chunk<T>();
            if constexpr (C::KONE)
                *reinterpret_cast<u32x4*>(lds + buf * 2 * C::TILE + r * C::RS + (D / C::VEC) * 16) = one_chunk<T>();
        }
    }
}

// Which row of K and V key position j of an attention is.  RowsInOrder: row j, the contiguous rows every kernel but the region
// tail reads (tile_load's code for it is the code it had before there was a choice).  RowsListed: row list[j], the ascending token
// list of a region (regions.hip) -- one index load per staged chunk pair, and the chunk's column taken back out of goff.
struct RowsInOrder { static constexpr bool LISTED = false, WEIGHTED = false; struct Table {}; };
struct RowsListed { static constexpr bool LISTED = true, WEIGHTED = false; const int32_t* list; struct Table {}; };

// What attend adds to the logit of key position j before the softmax looks at it.  NoKeyBias: nothing -- every line of the hook is
// under `if constexpr`, so an instantiation without a bias has the program text it had before there was a choice.  KeyBiasLog2:
// lb[j], in the log2 units of the pre-scaled logits (soft_regions.hip: log2 of the key token's weight, <= 0 and finite), indexed by
// key position; lb is 16-byte aligned and readable up to the end of the last 64-key tile.
struct NoKeyBias { static constexpr bool BIASED = false; };
struct KeyBiasLog2 { static constexpr bool BIASED = true; const float* lb; };
// RowsWeighted (soft_regions.hip, soft_matrix.hip): RowsListed's rows, each with a byte weight m in 1 .. 255 -- lb[j] = log2(m / 255) of the image's
// listed token j, the bias of key position j.  Table: the same for every image of a call, and the bytes themselves on the token grid
// (the tails take a query row's weight from them).
struct RowsWeighted {
    static constexpr bool LISTED = true, WEIGHTED = true;
    const int32_t* list;
    const float* lb;
    struct Table { const float* lb; const uint8_t* bytes; int stride; };      // lb [n_feat][stride], bytes [n_feat][N]
};
template <typename Rows>
__device__ __forceinline__ auto key_bias(const Rows& rows) {
    if constexpr (Rows::WEIGHTED) return KeyBiasLog2{rows.lb};
    else return NoKeyBias{};
}

template <typename T, int D, typename Rows = RowsInOrder>
__device__ __forceinline__ void tile_load(StageRegs<T, D>& sr, const T* kb, const T* vb, int ldk, int kv0, int Nk, Rows rows = Rows()) {
    typedef StageRegs<T, D> SR;
    const T* kt = kb + (size_t)kv0 * ldk;
    const T* vt = vb + (size_t)kv0 * ldk;
#pragma unroll
    for (int i = 0; i < SR::N; ++i) {
        if (kv0 + sr.row[i] < Nk && sr.row[i] < KT) {
            if constexpr (Rows::LISTED) {
                const size_t o = (size_t)rows.list[kv0 + sr.row[i]] * ldk + (sr.goff[i] - (unsigned)sr.row[i] * (unsigned)ldk);
                sr.k[i] = *reinterpret_cast<const u32x4*>(kb + o);
                sr.v[i] = *reinterpret_cast<const u32x4*>(vb + o);
            } else {
                sr.k[i] = *reinterpret_cast<const u32x4*>(kt + sr.goff[i]);
                sr.v[i] = *reinterpret_cast<const u32x4*>(vt + sr.goff[i]);
            }
        }
    }
}
template <typename T, int D>
__device__ __forceinline__ void tile_store(char* lds, const StageRegs<T, D>& sr, int kv0, int Nk) {
    typedef StageRegs<T, D> SR;
#pragma unroll
    for (int i = 0; i < SR::N; ++i) {
        if (kv0 + sr.row[i] < Nk && sr.row[i] < KT) {
            *reinterpret_cast<u32x4*>(lds + sr.loff[i]) = sr.k[i];
            *reinterpret_cast<u32x4*>(lds + sr.lvoff[i]) = sr.v[i];
        }
    }
}

// One full attention of this wave's 32 query rows against Nk keys.  On return o[db][r] holds the
// NORMALISED output O^T[d = db*32 + (r&3)+8(r>>2)+4*half][q = lane&31].  All 256 threads of the
// workgroup must call it together (it contains workgroup barriers).
// FAST: the running maximum is fixed after key tile 0 -- the later tiles compute P = exp2(S - m) without looking at their
// scores at all (no row maximum, no re-base test, no rescale: a third of the loop's non-exp vector instructions).  Softmax is
// invariant to the reference point, so a row whose true maximum lies above m just carries P > 1 and larger sums (f32 / h16
// have the exponent range for it).  Only if the excess passes ~100 (log2 units) can exp2 overflow; the caller detects that from a
// non-finite or absurd denominator and re-runs the block with FAST = false (attend_checked).
// Rows: which rows of kb / vb the Nk key positions are (RowsInOrder: rows 0 .. Nk - 1).
// Bias: an additive term per key position (NoKeyBias: none).  KeyBiasLog2: s(q, j) += lb[j] right after the QK^T MFMAs, so the
// ragged-tile mask, the row maximum, the re-base and the exponentials all see the biased logit and need no change.  The 32 values a
// lane needs per tile are eight 16-byte loads, the same addresses across a lane half, from an array that stays in L2 (64 floats a
// tile); nothing is staged in LDS, so ACfg's LDS budget and occupancy are the unbiased ones.  KONE: a bias is <= 0, it can only
// lower a logit, so no row passes the re-base slack that would not have passed it unbiased.
template <typename T, int D, bool FAST = false, typename Rows = RowsInOrder, typename Bias = NoKeyBias>
__device__ __forceinline__ void attend(const QFrags<T, D>& qfr, const T* kb, const T* vb, int ldk, int Nk, char* lds,
                                       OAcc<T, D>& oacc, float* l_out = nullptr, Rows rows = Rows(), Bias bias = Bias()) {
    typedef ACfg<T, D> C;
    typedef typename FragOf<T>::type Frag;
    QFrags<T, D> qloc = qfr;    // (KONE writes -m into the spare d = D slot of its own copy)
    auto& qf = qloc.f;
    auto& o = oacc.b;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
#pragma unroll
    for (int db = 0; db < C::NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
    float m_run = 0.f;          // running row max (log2 units); meaningful after tile 0 (KONE: a h16 value)
    f32x16 minit;               // the S^T accumulators' start value: -m_run (KONE: 0, the maximum rides in Q's spare slot)
#pragma unroll
    for (int r = 0; r < 16; ++r) minit[r] = 0.f;
    float l_run = 0.f;          // used only when !ONES

    const int ntiles = (Nk + KT - 1) / KT;
    StageRegs<T, D> sr;
    __syncthreads();            // a previous attend() of this workgroup may still be reading the buffers
    tile_init<T, D>(sr, lds, ldk, Nk, tid);
    if constexpr (C::PIPE) tile_load<T, D>(sr, kb, vb, ldk, 0, Nk, rows);
    __syncthreads();
    char* const lds0 = lds;
    for (int kt = 0; kt < ntiles; ++kt) {
        if constexpr (C::PIPE) {
            // buffer (kt&1) was last read in iteration kt-2; every wave has passed barrier kt-1 since
            lds = lds0 + (kt & 1) * 2 * C::TILE;
            tile_store<T, D>(lds, sr, kt * KT, Nk);
            __syncthreads();
            if (kt + 1 < ntiles) tile_load<T, D>(sr, kb, vb, ldk, (kt + 1) * KT, Nk, rows);
        } else {
            __syncthreads();                               // previous tile fully consumed
            tile_load<T, D>(sr, kb, vb, ldk, kt * KT, Nk, rows);
            tile_store<T, D>(lds, sr, kt * KT, Nk);
            __syncthreads();
        }

        // ---- S'^T = K Q^T - m for the two 32-row kv blocks (accumulators start at -m) ----------
        f32x16 s[2];
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
            s[jb] = minit;                  // -m in every register (KONE: the constant 0): the first MFMA reads it as its C operand
            const char* krow = lds + (jb * 32 + l31) * C::RS + half * 8 * C::ES;
#pragma unroll
            for (int ks = 0; ks < C::NKS; ++ks) {
                Frag kf;
                lload_frag(kf, krow + ks * 16 * C::ES);
                mma(kf, qf[ks], s[jb]);
            }
        }
        if constexpr (Bias::BIASED) {
            // slot (jb, r = 4 g + e) is key kt*KT + jb*32 + e + 8 g + 4 half: four consecutive positions per load
            const float* lb = bias.lb + kt * KT + 4 * half;
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(lb + jb * 32 + 8 * g);
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[jb][4 * g + e] += b4[e];
                }
        }
        if (kt * KT + KT > Nk) {                           // ragged last tile only
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kv = kt * KT + jb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (kv >= Nk) s[jb][r] = -INFINITY;
                }
        }
        // ---- online softmax (per query column == per lane) ---------------------------------
        float tmax = -INFINITY;
        if (!FAST || kt == 0) {
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[jb][r]);
            tmax = max_halves(tmax);
        }
        // tmax is relative to m_run.  Tile 0 always re-bases; later tiles only when some row's max
        // grew (the running max settles after a few tiles) -- exact, not a threshold.
        // (KONE re-bases only past a slack of 0.5, so that rounding m to h16 cannot leave a row just above 0 and
        // re-trigger on every tile; P <= 1.42 there)
        constexpr float SLACK = C::KONE ? 0.5f : 0.f;
        if (kt == 0 || (!FAST && !__all(tmax <= SLACK))) {
            float delta = kt == 0 ? tmax : fmaxf(tmax, 0.f);
            if constexpr (C::KONE) {
                if constexpr (sizeof(T) == 2) {
                    const float m_new = (float)(h16)(m_run + delta);      // the value Q can carry exactly
                    delta = m_new - m_run;
                    m_run = m_new;
                    if (half == 1) qf[C::NKS - 1][0] = (h16)(-m_new);       // d = D lives in element 0 of the upper half
                }
            } else {
                m_run += delta;
#pragma unroll
                for (int r = 0; r < 16; ++r) minit[r] = -m_run;
            }
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int r = 0; r < 16; ++r) s[jb][r] -= delta;
            if (kt != 0) {
                const float alpha = __builtin_amdgcn_exp2f(-delta);
                l_run *= alpha;
#pragma unroll
                for (int db = 0; db < C::NDB; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
            }
        }
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[jb][r] = __builtin_amdgcn_exp2f(s[jb][r]);
        if constexpr (!C::ONES) {
            float psum = 0.f;
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int r = 0; r < 16; ++r) psum += s[jb][r];
            l_run += psum;
        }

        // ---- O^T += V^T P^T ---------------------------------------------------------------
        const char* vt = lds + C::TILEK;
        if constexpr (sizeof(T) == 2) {
            // transposed read: per 16-lane group a 4x16 block; lane 4q+p supplies row q, cols 4p..4p+3
            const int i16 = lane & 15, g = lane >> 4;
            const int trow = 4 * (g >> 1) + (i16 >> 2);            // 4*half + q'
            const int tcol = 16 * (g & 1) + 4 * (i16 & 3);
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    h16x8 pf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[j] = (h16)s[jb][8 * s2 + j];
                    const char* vbase = vt + (jb * 32 + 16 * s2 + trow) * C::RSV + tcol * 2;
#pragma unroll
                    for (int db = 0; db < C::NDB; ++db) {
                        const char* pa = vbase + db * 64;
                        h16x4 lo = h16_ds_read_tr16_b64((pa));
                        h16x4 hi = h16_ds_read_tr16_b64((pa + 8 * C::RSV));
                        h16x8 vf;
#pragma unroll
                        for (int j = 0; j < 4; ++j) { vf[j] = lo[j]; vf[4 + j] = hi[j]; }
                        o[db] = H16_MFMA_32x32x16(vf, pf, o[db], 0, 0, 0);
                    }
                }
            }
        } else {
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = jb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    const char* vrow = vt + row * C::RSV + l31 * 4;
#pragma unroll
                    for (int db = 0; db < C::NDB; ++db) {
                        const float a = *reinterpret_cast<const float*>(vrow + db * 128);
                        o[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, s[jb][r], o[db], 0, 0, 0);
                    }
                }
            }
        }
    }
    float l_tot;
    if constexpr (C::ONES) {
        // row D of O^T = sum(P): block D/32, in-block row D%32 = (r&3)+8(r>>2)+4*half
        constexpr int RB = D / 32, RR = D % 32;
        constexpr int RH = (RR >> 2) & 1, REG = (RR & 3) + 4 * (RR >> 3);
        const float mine = o[RB][REG];
        const float other = __shfl_xor(mine, 32);
        l_tot = (half == RH) ? mine : other;
    } else {
        l_tot = l_run + __shfl_xor(l_run, 32);
    }
    if (l_out) *l_out = l_tot;
    const float inv = 1.0f / l_tot;
#pragma unroll
    for (int db = 0; db < C::NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] *= inv;
}

// ---- un-rescaled logits (align.hip, textattn.hip): S^T = K Q^T from the stored values, the softmax scale applied in f32 afterwards ----
// this lane's query row as un-scaled fragments (d >= D: zeros)
template <typename T, int D>
__device__ __forceinline__ void align_load_q(QFrags<T, D>& qf, const T* qrow, int half) {
#pragma unroll
    for (int ks = 0; ks < ACfg<T, D>::NKS; ++ks) {
        const int d0 = 16 * ks + 8 * half;
        if (d0 < D) {
            if constexpr (sizeof(T) == 2) qf.f[ks] = *reinterpret_cast<const h16x8*>(qrow + d0);
            else {
                qf.f[ks].lo = *reinterpret_cast<const f32x4*>(qrow + d0);
                qf.f[ks].hi = *reinterpret_cast<const f32x4*>(qrow + d0 + 4);
            }
        } else zero_frag(qf.f[ks]);
    }
}

// S^T = K Q^T of 32-key block jb of the staged tile against this wave's 32 query rows, raw (no scale, accumulators from 0):
// s[r] = Q[lane & 31] . K[jb * 32 + (r & 3) + 8 (r >> 2) + 4 half].  The one logit routine of align.hip's two passes and of
// text_attn_kernel (which stages up to four blocks, 128 keys).
template <typename T, int D>
__device__ __forceinline__ f32x16 align_logits(const QFrags<T, D>& qf, const char* lds, int jb, int l31, int half) {
    typedef ACfg<T, D> C;
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    const char* krow = lds + (jb * 32 + l31) * C::RS + half * 8 * C::ES;
#pragma unroll
    for (int ks = 0; ks < C::NKS; ++ks) {
        typename FragOf<T>::type kf;
        lload_frag(kf, krow + ks * 16 * C::ES);
        mma(kf, qf.f[ks], s);
    }
    return s;
}

// the key of accumulator slot (jb, r) in this lane's half
__device__ __forceinline__ int align_key(int jb, int r, int half) { return jb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half; }

inline float scale_log2_of(int D) { return (1.0f / sqrtf((float)D)) * 1.4426950408889634f; }

// head dims of the supported graphs: SD1.5 40/80/160, SDXL 64, DiT-XL/2 72, test configs 16/32/64
#define DSIM_FOR_EACH_D(X) X(16) X(32) X(40) X(64) X(72) X(80) X(160)

// f(std::integral_constant<int, D>()) for a head dim D of DSIM_FOR_EACH_D; DSIM_ERR_INVALID for any other
template <typename F>
int with_head_dim(int D, F&& f) {
    switch (D) {
#define X(d) case d: return f(std::integral_constant<int, d>());
        DSIM_FOR_EACH_D(X)
#undef X
        default: return DSIM_ERR_INVALID;
    }
}

}  // namespace
}  // namespace dsim
