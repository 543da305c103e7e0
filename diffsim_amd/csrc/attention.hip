// Flash-style attention for gfx950: the U-Net / DiT attention kernels on the tiled core (attn_core.h) and their dispatch.
//
//  * attn_kernel     : softmax(Q K^T / sqrt(D)) V for the U-Net's self/cross attention layers
//                      (replaces F.scaled_dot_product_attention inside diffusers' AttnProcessor2_0,
//                      restated at /root/reference/diffsim/hacked_attn.py:74-83).
//  * attn_q2_kernel, attn_long_kernel, attn_short_kernel: its forms for two query blocks per wave, long and short key
//                      sequences; attention_kernel() picks one.  The fused score tails on the same core are tails.hip's.
#include "attn_core.h"

namespace dsim {
namespace {

// One wave's 32 output rows from its O^T accumulators.  A lane owns one query row and, per 32-wide block db, the 8-byte chunks
// d = 32 db + 8 g + 4 half + (0..3): stored as they lie, a wave instruction writes 16 bytes into each of 32 rows -- 32 cache-line
// operations for 512 bytes, and the texture path, not HBM, sets the time (a 77-key cross-attention spent 0.29 of its 0.49 ms on
// them: profiles/r06_experiments.txt item 4).  The two halves of the wave therefore exchange every other chunk first (one
// v_permlane32_swap per register; both lanes of a pair belong to the same row), each lane stores 16 contiguous bytes, and the
// row gets 32 bytes per instruction from half as many instructions.  val(db, r) = the value to store for accumulator register r.
template <int D, typename F>
__device__ __forceinline__ void store_o_rows(h16* orow, int half, bool wide, F&& val) {
    constexpr int NDB = (D + 31) / 32;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    if (wide) {
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
                const int d0 = db * 32 + 16 * gp;
                if (d0 < D) {
                    unsigned a[2], b[2];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const h16x2 va = __builtin_convertvector((f32x2){val(db, 8 * gp + 2 * e), val(db, 8 * gp + 2 * e + 1)}, h16x2);
                        const h16x2 vb = __builtin_convertvector((f32x2){val(db, 8 * gp + 4 + 2 * e), val(db, 8 * gp + 4 + 2 * e + 1)}, h16x2);
                        a[e] = __builtin_bit_cast(unsigned, va);
                        b[e] = __builtin_bit_cast(unsigned, vb);
                    }
                    // lower lanes keep chunk 2 gp and receive the partner's; upper lanes keep chunk 2 gp + 1 and receive the partner's
                    const auto r0 = __builtin_amdgcn_permlane32_swap(a[0], b[0], false, false);
                    const auto r1 = __builtin_amdgcn_permlane32_swap(a[1], b[1], false, false);
                    const u32x4 w = {r0[0], r1[0], r0[1], r1[1]};
                    const int d = d0 + 8 * half;
                    if (d < D) *reinterpret_cast<u32x4*>(orow + d) = w;
                }
            }
    } else {
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = db * 32 + 8 * g + 4 * half;
                if (d < D) {
                    h16x4 v4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v4[j] = (h16)val(db, 4 * g + j);
                    *reinterpret_cast<h16x4*>(orow + d) = v4;
                }
            }
    }
}
// 16-byte row segments need 16-byte aligned rows
__device__ __forceinline__ bool wide_rows(const AttnArgs& p) { return p.ldo % 8 == 0 && ((size_t)p.out & 15) == 0; }

// attend() for TWO 32-row query blocks per wave (a workgroup = 256 queries): every K and V^T fragment read from LDS feeds both
// blocks.  attend() reads one kilobyte of fragments per MFMA -- at full MFMA rate 256 B per clock per CU, twice the LDS port -- so
// the one-block form tops out near half the matrix rate whatever else it does; this one halves the reads and the K / V staging per
// query.  Same arithmetic per row as attend() (same tiles, same order): results are bit-identical to it.  16-bit types without the
// K ones-column trick (d = 64: SDXL), double-buffered staging.
template <typename T, int D, bool FAST>
__device__ __forceinline__ void attend2(const QFrags<T, D> (&qfr)[2], const T* kb, const T* vb, int ldk, int Nk, char* lds,
                                        OAcc<T, D> (&oacc)[2], float (&l_out)[2]) {
    typedef ACfg<T, D> C;
    static_assert(sizeof(T) == 2 && C::PIPE && !C::KONE, "attend2: 16-bit, double-buffered, no K ones column");
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    float m_run[2] = {0.f, 0.f}, l_run[2] = {0.f, 0.f};
    f32x16 minit[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int db = 0; db < C::NDB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[q].b[db][r] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) minit[q][r] = 0.f;
    }
    const int ntiles = (Nk + KT - 1) / KT;
    StageRegs<T, D> sr;
    __syncthreads();
    tile_init<T, D>(sr, lds, ldk, Nk, tid);
    tile_load<T, D>(sr, kb, vb, ldk, 0, Nk);
    __syncthreads();
    char* const lds0 = lds;
    const int i16 = lane & 15, g = lane >> 4;
    const int trow = 4 * (g >> 1) + (i16 >> 2), tcol = 16 * (g & 1) + 4 * (i16 & 3);
    for (int kt = 0; kt < ntiles; ++kt) {
        lds = lds0 + (kt & 1) * 2 * C::TILE;
        tile_store<T, D>(lds, sr, kt * KT, Nk);
        __syncthreads();
        if (kt + 1 < ntiles) tile_load<T, D>(sr, kb, vb, ldk, (kt + 1) * KT, Nk);
        f32x16 s[2][2];
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
            s[0][jb] = minit[0];
            s[1][jb] = minit[1];
            const char* krow = lds + (jb * 32 + l31) * C::RS + half * 8 * C::ES;
#pragma unroll
            for (int ks = 0; ks < C::NKS; ++ks) {
                h16x8 kf;
                lload_frag(kf, krow + ks * 16 * C::ES);
                mma(kf, qfr[0].f[ks], s[0][jb]);
                mma(kf, qfr[1].f[ks], s[1][jb]);
            }
        }
        if (kt * KT + KT > Nk) {                           // ragged last tile only
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int kv = kt * KT + jb * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                        if (kv >= Nk) s[q][jb][r] = -INFINITY;
                    }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float tmax = -INFINITY;
            if (!FAST || kt == 0) {
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[q][jb][r]);
                tmax = max_halves(tmax);
            }
            if (kt == 0 || (!FAST && !__all(tmax <= 0.f))) {
                const float delta = kt == 0 ? tmax : fmaxf(tmax, 0.f);
                m_run[q] += delta;
#pragma unroll
                for (int r = 0; r < 16; ++r) minit[q][r] = -m_run[q];
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) s[q][jb][r] -= delta;
                if (kt != 0) {
                    const float alpha = __builtin_amdgcn_exp2f(-delta);
                    l_run[q] *= alpha;
#pragma unroll
                    for (int db = 0; db < C::NDB; ++db)
#pragma unroll
                        for (int r = 0; r < 16; ++r) oacc[q].b[db][r] *= alpha;
                }
            }
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int r = 0; r < 16; ++r) s[q][jb][r] = __builtin_amdgcn_exp2f(s[q][jb][r]);
            if constexpr (!C::ONES) {
                float psum = 0.f;
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) psum += s[q][jb][r];
                l_run[q] += psum;
            }
        }
        const char* vt = lds + C::TILEK;
#pragma unroll
        for (int jb = 0; jb < 2; ++jb) {
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                h16x8 pf[2];
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[q][j] = (h16)s[q][jb][8 * s2 + j];
                const char* vbase = vt + (jb * 32 + 16 * s2 + trow) * C::RSV + tcol * 2;
#pragma unroll
                for (int db = 0; db < C::NDB; ++db) {
                    const char* pa = vbase + db * 64;
                    const h16x4 lo = h16_ds_read_tr16_b64((pa));
                    const h16x4 hi = h16_ds_read_tr16_b64((pa + 8 * C::RSV));
                    h16x8 vf;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { vf[j] = lo[j]; vf[4 + j] = hi[j]; }
                    oacc[0].b[db] = H16_MFMA_32x32x16(vf, pf[0], oacc[0].b[db], 0, 0, 0);
                    oacc[1].b[db] = H16_MFMA_32x32x16(vf, pf[1], oacc[1].b[db], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        auto& o = oacc[q].b;
        float l_tot;
        if constexpr (C::ONES) {
            constexpr int RB = D / 32, RR = D % 32;
            constexpr int RH = (RR >> 2) & 1, REG = (RR & 3) + 4 * (RR >> 3);
            const float mine = o[RB][REG];
            const float other = __shfl_xor(mine, 32);
            l_tot = (half == RH) ? mine : other;
        } else {
            l_tot = l_run[q] + __shfl_xor(l_run[q], 32);
        }
        l_out[q] = l_tot;
        const float inv = 1.0f / l_tot;
#pragma unroll
        for (int db = 0; db < C::NDB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] *= inv;
    }
}

// The fast form, checked: every row's denominator must be finite and sane (it is >= ~1 by construction: the row's own
// tile-0 maximum contributes exp2(0)); otherwise some exp2 overflowed and the whole workgroup repeats the block exactly.
// h16 only (the fp32 parity mode keeps the exact running maximum).
template <typename T, int D, bool FASTK>
__device__ __forceinline__ void attend_checked(const QFrags<T, D>& qfr, const T* kb, const T* vb, int ldk, int Nk, char* lds,
                                               OAcc<T, D>& oacc) {
    if constexpr (sizeof(T) == 2 && FASTK) {
        float l = 0.f;
        attend<T, D, true>(qfr, kb, vb, ldk, Nk, lds, oacc, &l);
        // workgroup-uniform decision (attend() contains workgroup barriers): any wave with a bad row sends everybody back
        const int bad = !(l > 0.25f && l < DSIM_H16_LSUM_MAX);
        if (__syncthreads_or(bad)) attend<T, D, false>(qfr, kb, vb, ldk, Nk, lds, oacc);
    } else {
        attend<T, D, false>(qfr, kb, vb, ldk, Nk, lds, oacc);
    }
}

// ---- long key sequences: two query blocks per wave, software-pipelined ---------------------------------------------------
// The 64 x 64 self-attention (4096 keys, d = 40) keeps the MFMA pipe 55 % and the VALU 57 % busy in attn_kernel, but only
// 22 % of the time both at once (r03 counters): within a wave the tile body is serial -- QK^T MFMAs, then 32 v_exp per lane,
// then PV MFMAs -- and the other waves of the SIMD are as likely to be in the same phase as in the complementary one.
// Here the overlap is built into ONE wave's instruction stream.  A wave owns 64 query rows as two 32-column blocks; a key
// tile is four "units" (query block q, key half j), each QK (NKS MFMAs) -> softmax (16 v_exp + 8 v_cvt_pk per lane) -> PV
// (2 NDB MFMAs).  The units run as a three-stage pipeline, one step per unit:
//     step n:   MFMA pipe: PV(unit n-1), QK(unit n+1)     VALU: softmax(unit n)
// with the v_exp / v_cvt of unit n issued between the MFMAs (pinned by sched_barrier), so the matrix pipe executes while
// the VALU converts.  The pipeline crosses tile borders (the last step of tile t starts tile t + 1's first QK and the first
// step of tile t + 1 finishes tile t's last PV), so three K/V tiles are live: a 3-deep LDS ring (58 KB, two workgroups per
// CU), one barrier per tile.  h16, fixed-reference softmax (attend<.., FAST>: the maximum of key tile 0), Nk % 64 == 0.
// DBG: kbench ablation masks (1 no v_exp, 2 no PV MFMAs, 4 no QK MFMAs, 8 no global loads in the loop, 16 no v_cvt); 0 in the product
template <int D, int DBG = 0>
__device__ __forceinline__ void attend_pipelined2(const QFrags<h16, D> (&qfr)[2], const h16* kb, const h16* vb, int ldk, int Nk,
                                                  char* lds0, OAcc<h16, D> (&oacc)[2], float (&l_out)[2]) {
    typedef h16 T;
    typedef ACfg<T, D> C;
    constexpr int BUF = 2 * C::TILE;                // one K tile + one V tile
    constexpr int NM = 2 * C::NDB + C::NKS;         // MFMAs per step
    QFrags<T, D> qloc[2] = {qfr[0], qfr[1]};
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const int i16 = lane & 15, g4 = lane >> 4;
    const int koff = l31 * C::RS + half * 16;                                                   // K fragment row of this lane
    const int voff = C::TILEK + (4 * (g4 >> 1) + (i16 >> 2)) * C::RSV + (16 * (g4 & 1) + 4 * (i16 & 3)) * 2;   // transposed V read
    f32x16 minit[2];
    float l_run[2] = {0.f, 0.f};
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
#pragma unroll
        for (int db = 0; db < C::NDB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[qb].b[db][r] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) minit[qb][r] = 0.f;
    }
    const int ntiles = Nk / KT;
    StageRegs<T, D> sr;
    __syncthreads();            // a previous user of the buffers (the exact fallback never runs before this)
    {
        // ring init: zero padding columns, the ones column of V (row sums out of the PV MFMAs) and of K (KONE)
        typedef StageRegs<T, D> SR;
        const u32x4 z = {0u, 0u, 0u, 0u};
        if (D < C::DPL)
            for (int o = tid * 16; o < 3 * BUF; o += 256 * 16) *reinterpret_cast<u32x4*>(lds0 + o) = z;
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
            for (int i = tid; i < KT * 3; i += 256) {
                const int buf = i / KT, r = i - buf * KT;
                *reinterpret_cast<u32x4*>(lds0 + buf * BUF + C::TILEK + r * C::RSV + (D / C::VEC) * 16) = one_chunk<T>();
                if constexpr (C::KONE) *reinterpret_cast<u32x4*>(lds0 + buf * BUF + r * C::RS + (D / C::VEC) * 16) = one_chunk<T>();
            }
        }
    }
    // Nk % KT == 0: every tile is whole, so the staging needs no per-row bounds test -- the only predicate left is "this thread
    // has a chunk in round i" (KT * CPRD chunks over 256 threads), which is WAVE-uniform (a scalar branch, no exec masking).
    // Past the end the last tile is refetched into a dead ring slot.
    constexpr int NCH = KT * StageRegs<T, D>::CPRD;
    static_assert(NCH % 64 == 0, "whole waves per staging round");
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    auto stage_load = [&](int t) {
        const int tt = t < ntiles ? t : ntiles - 1;
        const T* kt = kb + (size_t)tt * KT * ldk;
        const T* vt = vb + (size_t)tt * KT * ldk;
#pragma unroll
        for (int i = 0; i < StageRegs<T, D>::N; ++i)
            if (i * 256 + wv * 64 < NCH) {
                sr.k[i] = *reinterpret_cast<const u32x4*>(kt + sr.goff[i]);
                sr.v[i] = *reinterpret_cast<const u32x4*>(vt + sr.goff[i]);
            }
    };
    auto stage_store = [&](char* buf) {
#pragma unroll
        for (int i = 0; i < StageRegs<T, D>::N; ++i)
            if (i * 256 + wv * 64 < NCH) {
                *reinterpret_cast<u32x4*>(buf + sr.loff[i]) = sr.k[i];
                *reinterpret_cast<u32x4*>(buf + sr.lvoff[i]) = sr.v[i];
            }
    };
    stage_load(0);
    __syncthreads();
    stage_store(lds0);
    stage_load(1);
    __syncthreads();

    auto qk = [&](const char* buf, int q, int j, f32x16& s) {            // S'^T block of unit (q, j)
        s = minit[q];
#pragma unroll
        for (int ks = 0; ks < C::NKS; ++ks) {
            const h16x8 kf = *reinterpret_cast<const h16x8*>(buf + koff + j * 32 * C::RS + ks * 32);
            mma(kf, qloc[q].f[ks], s);
        }
    };
    auto vfrag = [&](const char* buf, int j, int s2, int db) {
        const char* pa = buf + voff + (j * 32 + 16 * s2) * C::RSV + db * 64;
        const h16x4 lo = h16_ds_read_tr16_b64((pa));
        const h16x4 hi = h16_ds_read_tr16_b64((pa + 8 * C::RSV));
        h16x8 vf;
#pragma unroll
        for (int e = 0; e < 4; ++e) { vf[e] = lo[e]; vf[4 + e] = hi[e]; }
        return vf;
    };
    auto pv = [&](const char* buf, int q, int j, const h16x8 (&pf)[2]) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int db = 0; db < C::NDB; ++db)
                oacc[q].b[db] = H16_MFMA_32x32x16(vfrag(buf, j, s2, db), pf[s2], oacc[q].b[db], 0, 0, 0);
    };
    auto softmax = [&](int q, f32x16& s, h16x8 (&pf)[2]) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_exp2f(s[r]);
        if constexpr (!C::ONES) {
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) psum += s[r];
            l_run[q] += psum;
        }
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int e = 0; e < 8; ++e) pf[f][e] = (h16)s[8 * f + e];
    };

    // ---- key tile 0, unpipelined: it fixes every row's reference point -------------------------------------------------
    h16x8 pfA[2], pfB[2];
    f32x16 sA, sB;
    {
        f32x16 s0[2][2];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int j = 0; j < 2; ++j) qk(lds0, q, j, s0[q][j]);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float tmax = -INFINITY;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s0[q][j][r]);
            tmax = max_halves(tmax);
            float delta = tmax;
            if constexpr (C::KONE) {
                const float m_new = (float)(h16)delta;            // the value Q's spare slot carries exactly
                delta = m_new;
                if (half == 1) qloc[q].f[C::NKS - 1][0] = (h16)(-m_new);
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) minit[q][r] = -delta;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) s0[q][j][r] -= delta;
        }
        h16x8 pft[2];
        softmax(0, s0[0][0], pft); pv(lds0, 0, 0, pft);
        softmax(0, s0[0][1], pft); pv(lds0, 0, 1, pft);
        softmax(1, s0[1][0], pft); pv(lds0, 1, 0, pft);
        softmax(1, s0[1][1], pfB);                          // its PV is the first step's
    }
    // The four steps of a tile need only two fragment sets: steps 1 and 2 share X = {V^T(t, j0), K(t, j1)}, step 3 and the
    // next tile's step 0 share Y = {V^T(t, j1), K(t + 1, j0)}.  Each is read from LDS ONE step before its first use (X during
    // step 0, Y during step 2), so no MFMA waits on an LDS round trip and every fragment read feeds two query blocks.
    struct FragSet { h16x8 vf[2][C::NDB]; h16x8 kf[C::NKS]; };
    auto load_set = [&](FragSet& F, const char* vbuf, int pj, const char* kbuf, int kj) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int db = 0; db < C::NDB; ++db) F.vf[s2][db] = vfrag(vbuf, pj, s2, db);
#pragma unroll
        for (int ks = 0; ks < C::NKS; ++ks) F.kf[ks] = *reinterpret_cast<const h16x8*>(kbuf + koff + kj * 32 * C::RS + ks * 32);
    };
    FragSet X, Y;
    // tile 1 becomes visible, tile 2 is on its way; the pipeline's first QK
    stage_store(lds0 + BUF);
    stage_load(2);
    __syncthreads();
    load_set(Y, lds0, 1, lds0 + BUF, 0);
    sA = minit[0];
#pragma unroll
    for (int ks = 0; ks < C::NKS; ++ks) mma(Y.kf[ks], qloc[0].f[ks], sA);

    // One pipeline step: the MFMAs of PV(query block pq; P fragments pin; V^T fragments F.vf) and of QK(query block kq; F.kf)
    // -> sout, with the softmax of sin -> pout (a unit of query block sq) issued between them.
    auto step = [&](const FragSet& F, int pq, const h16x8 (&pin)[2], int kq, f32x16& sout, int sq, f32x16& sin, h16x8 (&pout)[2]) {
        __builtin_amdgcn_sched_barrier(0);
        constexpr int EPG = (DBG & 96) == 32 ? 4 : ((DBG & 96) == 64 ? 6 : ((DBG & 96) == 96 ? 8 : (16 + NM - 2) / (NM - 1)));       // v_exp per MFMA over the first NM - 1 groups
#pragma unroll
        for (int g = 0; g < NM; ++g) {
            // QK first: its result is the NEXT step's softmax input (a whole PV group of slack), and the P fragments this step's
            // PV reads were converted a QK group ago
            if (g >= C::NKS) {
                const int s2 = (g - C::NKS) / C::NDB, db = (g - C::NKS) % C::NDB;
                if (!(DBG & 2)) oacc[pq].b[db] = H16_MFMA_32x32x16(F.vf[s2][db], pin[s2], oacc[pq].b[db], 0, 0, 0);
            } else {
                const int ks = g;
                if (DBG & 4) { if (ks == 0) sout = minit[kq]; }
                else if (ks == 0) sout = H16_MFMA_32x32x16(F.kf[0], qloc[kq].f[0], minit[kq], 0, 0, 0);
                else sout = H16_MFMA_32x32x16(F.kf[ks], qloc[kq].f[ks], sout, 0, 0, 0);
            }
#pragma unroll
            for (int r = g * EPG; r < (g + 1) * EPG && r < 16; ++r)
                if (!(DBG & 1)) sin[r] = __builtin_amdgcn_exp2f(sin[r]);
            // the conversions of a P fragment follow its eight exponentials
#pragma unroll
            for (int f = 0; f < 2; ++f)
                if ((g == (8 * f + 7) / EPG + 1) || (g == NM - 1 && (8 * f + 7) / EPG + 1 > NM - 1)) {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (!(DBG & 16)) pout[f][e] = (h16)sin[8 * f + e];
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (!C::ONES) {
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) psum += sin[r];
            l_run[sq] += psum;
        }
    };

    const char* bprev = lds0;              // tile t - 1
    const char* bcur = lds0 + BUF;         // tile t
    char* bnext = lds0 + 2 * BUF;          // tile t + 1
    for (int t = 1; t < ntiles; ++t) {
        // tile t + 1 into the ring slot tile t - 2 left (its last reader was the Y load of iteration t - 2, two barriers
        // ago); rows past Nk are never stored, and the last iteration's QK of "tile ntiles" reads stale finite data whose
        // result nobody uses
        stage_store(bnext);
        if (!(DBG & 8)) stage_load(t + 2);
        __syncthreads();
        load_set(X, bcur, 0, bcur, 1);
        step(Y, 1, pfB, 1, sB, 0, sA, pfA);       // PV(q1, j1, t - 1)   QK(q1, j0, t)       softmax(q0, j0, t)
        step(X, 0, pfA, 0, sA, 1, sB, pfB);       // PV(q0, j0, t)       QK(q0, j1, t)       softmax(q1, j0, t)
        load_set(Y, bcur, 1, bnext, 0);
        step(X, 1, pfB, 1, sB, 0, sA, pfA);       // PV(q1, j0, t)       QK(q1, j1, t)       softmax(q0, j1, t)
        step(Y, 0, pfA, 0, sA, 1, sB, pfB);       // PV(q0, j1, t)       QK(q0, j0, t + 1)   softmax(q1, j1, t)
        const char* tmp = bprev;
        bprev = bcur; bcur = bnext; bnext = const_cast<char*>(tmp);
    }
    // the last tile's last unit: PV(q1, j1) from the Y fragments
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int db = 0; db < C::NDB; ++db)
            oacc[1].b[db] = H16_MFMA_32x32x16(Y.vf[s2][db], pfB[s2], oacc[1].b[db], 0, 0, 0);
    (void)bprev;

#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        auto& o = oacc[qb].b;
        float l_tot;
        if constexpr (C::ONES) {
            constexpr int RB = D / 32, RR = D % 32;
            constexpr int RH = (RR >> 2) & 1, REG = (RR & 3) + 4 * (RR >> 3);
            const float mine = o[RB][REG];
            const float other = __shfl_xor(mine, 32);
            l_tot = (half == RH) ? mine : other;
        } else {
            l_tot = l_run[qb] + __shfl_xor(l_run[qb], 32);
        }
        l_out[qb] = l_tot;
        const float inv = 1.0f / l_tot;
#pragma unroll
        for (int db = 0; db < C::NDB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] *= inv;
    }
}

// grid ceil(Nq/256) * H * B (1-D): a workgroup = 4 waves x 64 query rows
template <int D, int DBG>
__global__ __launch_bounds__(256, 2) void attn_long_kernel(const AttnArgs p, const float scale_log2) {
    typedef h16 T;
    typedef ACfg<T, D> C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int nqb = (p.Nq + 255) / 256;
    int bid = blockIdx.x;
    if (p.xcd_remap) {          // as attn_kernel: the query blocks of one (batch, head) run on one XCD back to back
        const int nwg = gridDim.x, xcd = bid & 7, qq = nwg >> 3, r = nwg & 7, slot = bid >> 3;
        bid = (xcd < r ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq) + slot;
    }
    const int qblk = bid % nqb, bh = bid / nqb;
    const int h = bh % p.H, b = bh / p.H;
    QFrags<T, D> qf[2];
    int q[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        q[qb] = qblk * 256 + wave * 64 + qb * 32 + l31;
        const int qc = q[qb] < p.Nq ? q[qb] : p.Nq - 1;
        load_q<T, D>(qf[qb], (const T*)p.q + ((size_t)b * p.Nq + qc) * p.ldq + h * D, half, scale_log2);
    }
    const size_t kvoff = (size_t)(b % p.Bkv) * p.Nk * p.ldk + h * D;
    OAcc<T, D> oa[2];
    float l[2];
    attend_pipelined2<D, DBG>(qf, (const T*)p.k + kvoff, (const T*)p.v + kvoff, p.ldk, p.Nk, smem, oa, l);
    // every row's denominator must be finite and sane (attend_checked): else the workgroup repeats the block exactly
    const int bad = !(l[0] > 0.25f && l[0] < DSIM_H16_LSUM_MAX) || !(l[1] > 0.25f && l[1] < DSIM_H16_LSUM_MAX);
    if (__syncthreads_or(bad)) {
        attend<T, D, false>(qf[0], (const T*)p.k + kvoff, (const T*)p.v + kvoff, p.ldk, p.Nk, smem, oa[0]);
        attend<T, D, false>(qf[1], (const T*)p.k + kvoff, (const T*)p.v + kvoff, p.ldk, p.Nk, smem, oa[1]);
    }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        if (q[qb] >= p.Nq) continue;
        T* orow = (T*)p.out + ((size_t)b * p.Nq + q[qb]) * p.ldo + h * D;
        store_o_rows<D>(orow, half, wide_rows(p), [&](int db, int r) { return oa[qb].b[db][r]; });
    }
}

// grid ceil(Nq/256) * H * B (1-D): attend2 -- a workgroup = 4 waves x 64 query rows (two 32-row blocks per wave)
template <int D, bool FASTK>
__global__ __launch_bounds__(256, 2) void attn_q2_kernel(const AttnArgs p, const float scale_log2) {
    typedef h16 T;
    typedef ACfg<T, D> C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int nqb = (p.Nq + 255) / 256;
    int bid = blockIdx.x;
    if (p.xcd_remap) {
        const int nwg = gridDim.x, xcd = bid & 7, qq = nwg >> 3, r = nwg & 7, slot = bid >> 3;
        bid = (xcd < r ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq) + slot;
    }
    const int qblk = bid % nqb, bh = bid / nqb;
    const int h = bh % p.H, b = bh / p.H;
    QFrags<T, D> qf[2];
    int q[2];
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        q[qb] = qblk * 256 + wave * 64 + qb * 32 + l31;
        const int qc = q[qb] < p.Nq ? q[qb] : p.Nq - 1;
        load_q<T, D>(qf[qb], (const T*)p.q + ((size_t)b * p.Nq + qc) * p.ldq + h * D, half, scale_log2);
    }
    const size_t kvoff = (size_t)(b % p.Bkv) * p.Nk * p.ldk + h * D;
    OAcc<T, D> oa[2];
    float l[2];
    attend2<T, D, FASTK>(qf, (const T*)p.k + kvoff, (const T*)p.v + kvoff, p.ldk, p.Nk, smem, oa, l);
    if constexpr (FASTK) {          // as attend_checked: a non-finite or absurd denominator sends the workgroup through the exact form
        const int bad = !(l[0] > 0.25f && l[0] < DSIM_H16_LSUM_MAX) || !(l[1] > 0.25f && l[1] < DSIM_H16_LSUM_MAX);
        if (__syncthreads_or(bad)) attend2<T, D, false>(qf, (const T*)p.k + kvoff, (const T*)p.v + kvoff, p.ldk, p.Nk, smem, oa, l);
    }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        if (q[qb] >= p.Nq) continue;
        T* orow = (T*)p.out + ((size_t)b * p.Nq + q[qb]) * p.ldo + h * D;
        store_o_rows<D>(orow, half, wide_rows(p), [&](int db, int r) { return oa[qb].b[db][r]; });
    }
}

// grid ceil(Nq/128) * H * B (1-D)
// FASTK: the fixed-reference softmax of attend<.., FAST> (long key sequences; see launch_attn_d)
template <typename T, int D, bool FASTK>
__global__ __launch_bounds__(256, (ACfg<T, D>::WPS)) void attn_kernel(const AttnArgs p, const float scale_log2) {
    typedef ACfg<T, D> C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    // 1-D grid, XCD-aware: workgroup ids go round-robin over the 8 XCDs, each with its own L2.  Give every XCD a
    // contiguous run of logical blocks so that the query blocks of one (batch, head) -- which all re-read the same
    // K and V -- run on ONE XCD back to back and find them in its L2 (bijective for any grid size).
    const int nqb = (p.Nq + 127) / 128;
    int bid = blockIdx.x;
    if (p.xcd_remap) {
        const int nwg = gridDim.x, xcd = bid & 7, qq = nwg >> 3, r = nwg & 7, slot = bid >> 3;
        bid = (xcd < r ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq) + slot;
    }
    const int qblk = bid % nqb, bh = bid / nqb;
    const int h = bh % p.H, b = bh / p.H;
    const int q = qblk * 128 + wave * 32 + l31;
    const int qc = q < p.Nq ? q : p.Nq - 1;
    const T* qrow = (const T*)p.q + ((size_t)b * p.Nq + qc) * p.ldq + h * D;
    QFrags<T, D> qf;
    load_q<T, D>(qf, qrow, half, scale_log2);
    const size_t kvoff = (size_t)(b % p.Bkv) * p.Nk * p.ldk + h * D;
    OAcc<T, D> oa;
    attend_checked<T, D, FASTK>(qf, (const T*)p.k + kvoff, (const T*)p.v + kvoff, p.ldk, p.Nk, smem, oa);
    auto& o = oa.b;
    if (q < p.Nq) {
        T* orow = (T*)p.out + ((size_t)b * p.Nq + q) * p.ldo + h * D;
        if constexpr (sizeof(T) == 2) {
            store_o_rows<D>((h16*)orow, half, wide_rows(p), [&](int db, int r) { return o[db][r]; });
        } else {
#pragma unroll
            for (int db = 0; db < C::NDB; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int d = db * 32 + 8 * g + 4 * half;
                    if (d < D) {
                        f32x4 v4;
#pragma unroll
                        for (int j = 0; j < 4; ++j) v4[j] = o[db][4 * g + j];
                        *reinterpret_cast<f32x4*>(orow + d) = v4;
                    }
                }
        }
    }
}

// ---- short key sequences (the 77-key prompt context of every cross-attention) -------------------------------------------
// attn_kernel spends most of such a launch around its two key tiles: 38 KB of LDS zero-fill, the staging of K and V, three
// barriers and an online-softmax loop whose second tile is four fifths padding -- per 128 queries, 65 536 workgroups at the
// 64 x 64 level (181 TF/s, 2.4 TB/s).  Here the keys (<= 96 = three 32-row blocks) are staged ONCE per workgroup and stay in
// LDS while the workgroup walks QIT query blocks of its (batch, head) with no barrier in the loop: per block three S^T tiles,
// ONE softmax pass with the exact row maximum (no running state), PV, normalise, store.  The launch becomes what its bytes say
// it is: a stream of Q in and O out.  h16; K / V images in attn_kernel's padded row-major layouts (ones column of V included).
// The heads of a token share cache lines in Q and O (80 bytes per head at d = 40): the XCD-aware block order that keeps the
// heads of a batch element on one XCD matters more than anything inside the loop (0.62 -> 0.46 ms at d = 40).
// Round 6 (profiles/r06_experiments.txt item 4): the loop was bound by its vector instructions (493 per 32-query block against 21
// MFMAs; vector pipe 0.46 busy, matrix pipe 0.14), so
//  - Q is NOT pre-scaled (24 multiplies + conversions per block): the softmax computes exp2(fma(s, c, -m c)) as packed v_pk_fma_f32;
//  - K80 (64 < Nk <= 80: the 77-key prompt context): the ragged third key block takes its -inf mask as eight loop-invariant
//    addends instead of 48 compares + selects per block (whose 48 lane masks hipcc kept in VGPR lanes: a v_readlane each), and
//    its dead upper half (keys 80-95) is never exponentiated or multiplied;
//  - a workgroup walks query blocks ACROSS the batch elements that share its K / V (b = bkv, bkv + Bkv, ...: the CFG halves of every
//    image read the same prompt), so the 256-query level of the U-Net (d = 160: two blocks per batch element) amortises its staging
//    over eight blocks like the others; block order [bkv][chunk][head]: the heads of a row stay neighbours on one XCD.
template <int D, bool K80>
__global__ __launch_bounds__(256, 2) void attn_short_kernel(const AttnArgs p, const float scale_log2, const int qit) {
    typedef h16 T;
    typedef ACfg<T, D> C;
    constexpr int KR = 96;                                   // key rows held (three 32-row MFMA blocks)
    constexpr int CPRD = D / C::VEC;                         // real 16-byte chunks per row
    constexpr int VOFF = KR * C::RS;                         // V image behind the K image
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
    const int nqb = (p.Nq + 127) / 128;                      // query blocks per batch element
    const int nbmax = (p.B + p.Bkv - 1) / p.Bkv;             // batch elements per K / V
    const int nch = (nbmax * nqb + qit - 1) / qit;           // chunks of qit blocks per (K / V, head)
    int bid = blockIdx.x;
    if (p.xcd_remap) {          // every XCD a contiguous run of (K / V, chunk, head) items -- the heads of a row share cache lines
        const int nwg = gridDim.x, xcd = bid & 7, qq = nwg >> 3, r = nwg & 7, slot = bid >> 3;
        bid = (xcd < r ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq) + slot;
    }
    const int h = bid % p.H, t0 = bid / p.H, ch = t0 % nch, bkv = t0 / nch;
    const int nbg = (p.B - bkv + p.Bkv - 1) / p.Bkv;         // batch elements that read this K / V
    if (ch * qit >= nbg * nqb) return;
    const size_t kvoff = (size_t)bkv * p.Nk * p.ldk + h * D;
    const T* kb = (const T*)p.k + kvoff;
    const T* vb = (const T*)p.v + kvoff;
    // ---- stage K and V once: zero image (padding columns, rows >= Nk), then the real chunks and V's ones column ---------
    {
        const u32x4 z = {0u, 0u, 0u, 0u};
        for (int o = tid * 16; o < KR * (C::RS + C::RSV); o += 256 * 16) *reinterpret_cast<u32x4*>(smem + o) = z;
        __syncthreads();
        for (int idx = tid; idx < p.Nk * CPRD; idx += 256) {
            const int r = idx / CPRD, c = idx - r * CPRD;
            const u32x4 kk = *reinterpret_cast<const u32x4*>(kb + (size_t)r * p.ldk + c * C::VEC);
            const u32x4 vv = *reinterpret_cast<const u32x4*>(vb + (size_t)r * p.ldk + c * C::VEC);
            *reinterpret_cast<u32x4*>(smem + r * C::RS + c * 16) = kk;
            *reinterpret_cast<u32x4*>(smem + VOFF + r * C::RSV + c * 16) = vv;
        }
        if constexpr (C::ONES)
            for (int r = tid; r < p.Nk; r += 256) *reinterpret_cast<u32x4*>(smem + VOFF + r * C::RSV + CPRD * 16) = one_chunk<T>();
        __syncthreads();
    }
    const int i16 = lane & 15, g4 = lane >> 4;
    const char* const kfr = smem + l31 * C::RS + half * 16;
    const char* const vfr = smem + VOFF + (4 * (g4 >> 1) + (i16 >> 2)) * C::RSV + (16 * (g4 & 1) + 4 * (i16 & 3)) * 2;
    // unscaled Q fragments of a block's 32 rows of this wave (rows past the end: the last row, never stored)
    auto load_q_raw = [&](QFrags<T, D>& f, int b, int q) {
        const int qq = q < p.Nq ? q : p.Nq - 1;
        const T* qrow = (const T*)p.q + ((size_t)b * p.Nq + qq) * p.ldq + h * D;
#pragma unroll
        for (int ks = 0; ks < C::NKS; ++ks) {
            const int d0 = 16 * ks + 8 * half;
            if (d0 < D) f.f[ks] = *reinterpret_cast<const h16x8*>(qrow + d0);
            else zero_frag(f.f[ks]);
        }
    };
    // K80: the third key block's mask as eight loop-invariant addends (key = 64 + (r & 3) + 8 (r >> 2) + 4 half; r >= 8 is dead)
    float bias[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) bias[r] = (64 + (r & 3) + 8 * (r >> 2) + 4 * half >= p.Nk) ? -INFINITY : 0.f;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 c2 = {scale_log2, scale_log2};
    const bool wide = wide_rows(p);

    int bi = (ch * qit) / nqb, qblk = ch * qit - bi * nqb;
    QFrags<T, D> qf;
    load_q_raw(qf, bi * p.Bkv + bkv, qblk * 128 + wave * 32 + l31);
    for (int it = 0; it < qit && bi < nbg; ++it) {
        const int b = bi * p.Bkv + bkv;
        const int q = qblk * 128 + wave * 32 + l31;
        if (++qblk == nqb) { qblk = 0; ++bi; }
        // the next block's Q rows fly while this block computes
        QFrags<T, D> qn;
        load_q_raw(qn, (bi < nbg ? bi : nbg - 1) * p.Bkv + bkv, qblk * 128 + wave * 32 + l31);
        if (q - l31 < p.Nq) {                               // wave-uniform: some of this wave's rows exist
            f32x16 s[3];
#pragma unroll
            for (int kbk = 0; kbk < 3; ++kbk) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[kbk][r] = 0.f;
#pragma unroll
                for (int ks = 0; ks < C::NKS; ++ks) {
                    h16x8 kf;
                    lload_frag(kf, kfr + kbk * 32 * C::RS + ks * 32);
                    mma(kf, qf.f[ks], s[kbk]);
                }
            }
            // exact row maximum over the (<= 96) keys: lane-local + one exchange between the halves
            float m = -INFINITY;
#pragma unroll
            for (int kbk = 0; kbk < 3; ++kbk)
#pragma unroll
                for (int r = 0; r < ((K80 && kbk == 2) ? 8 : 16); ++r) {
                    if constexpr (!K80) {
                        const int kv = kbk * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                        if (kv >= p.Nk) s[kbk][r] = -INFINITY;
                    } else if (kbk == 2) {
                        s[kbk][r] += bias[r];
                    }
                    m = fmaxf(m, s[kbk][r]);
                }
            m = max_halves(m);
            const float mc = -m * scale_log2;
            const f32x2 m2 = {mc, mc};
            float psum = 0.f;
#pragma unroll
            for (int kbk = 0; kbk < 3; ++kbk)
#pragma unroll
                for (int r = 0; r < ((K80 && kbk == 2) ? 8 : 16); r += 2) {
                    const f32x2 e = __builtin_elementwise_fma((f32x2){s[kbk][r], s[kbk][r + 1]}, c2, m2);
                    s[kbk][r] = __builtin_amdgcn_exp2f(e[0]);
                    s[kbk][r + 1] = __builtin_amdgcn_exp2f(e[1]);
                    if constexpr (!C::ONES) psum += s[kbk][r] + s[kbk][r + 1];
                }
            f32x16 o[C::NDB];
#pragma unroll
            for (int db = 0; db < C::NDB; ++db)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
#pragma unroll
            for (int kbk = 0; kbk < 3; ++kbk)
#pragma unroll
                for (int s2 = 0; s2 < ((K80 && kbk == 2) ? 1 : 2); ++s2) {
                    h16x8 pf;
#pragma unroll
                    for (int e = 0; e < 8; ++e) pf[e] = (h16)s[kbk][8 * s2 + e];
#pragma unroll
                    for (int db = 0; db < C::NDB; ++db) {
                        const char* pa = vfr + (kbk * 32 + 16 * s2) * C::RSV + db * 64;
                        const h16x4 lo = h16_ds_read_tr16_b64((pa));
                        const h16x4 hi = h16_ds_read_tr16_b64((pa + 8 * C::RSV));
                        h16x8 vf;
#pragma unroll
                        for (int e = 0; e < 4; ++e) { vf[e] = lo[e]; vf[4 + e] = hi[e]; }
                        o[db] = H16_MFMA_32x32x16(vf, pf, o[db], 0, 0, 0);
                    }
                }
            float l_tot;
            if constexpr (C::ONES) {
                constexpr int RB = D / 32, RR = D % 32;
                constexpr int RH = (RR >> 2) & 1, REG = (RR & 3) + 4 * (RR >> 3);
                const float mine = o[RB][REG];
                const float other = __shfl_xor(mine, 32);
                l_tot = (half == RH) ? mine : other;
            } else {
                l_tot = psum + __shfl_xor(psum, 32);
            }
            const float inv = 1.0f / l_tot;
            if (q < p.Nq) {
                T* orow = (T*)p.out + ((size_t)b * p.Nq + q) * p.ldo + h * D;
                store_o_rows<D>(orow, half, wide, [&](int db, int r) { return o[db][r] * inv; });
            }
        }
        qf = qn;
    }
}

// (AttnKernel, the kernels launch_attention starts: common.h)

// fewest keys that take the fixed-reference softmax: long key sequences (>= 1024 keys: the 64 x 64 and 32 x 32 self-attentions)
// run 6 % faster on it at 4096 keys x d = 40, 10 % at 1024 keys x d = 80, 14 % at 1024 keys x d = 64 (SDXL); short ones
// (cross-attention's 77 keys, the 16 x 16 level: 0.179 -> 0.195 ms at 256 keys x d = 160) keep the exact running maximum -- there
// the end-of-block check costs more than the skipped maxima save
constexpr int ATTN_FAST_MIN = 1024;

// The one place that decides which kernel serves a problem: launch_attention and attention_kernel_kind both follow it.
AttnKernel attention_kernel(const AttnArgs& a, int dtype) {
    if (dtype == DSIM_F32) return AttnKernel::Exact;
    if (sdpa160_applies(a)) return AttnKernel::P160;
    // the prompt context of the cross-attentions (77 keys): keys resident in LDS, several query blocks per workgroup
    // (round 6, interleaved A/B against the tiled kernel at 64 pairs: d = 40 0.492 -> 0.387 ms, d = 80 0.221 -> 0.199, d = 160 at
    //  256 queries 0.112 -> 0.091, SDXL's d = 64 at 4096 / 1024 queries 0.736 -> 0.652 / 0.397 -> 0.381)
    if ((a.D == 40 || a.D == 64 || a.D == 80 || a.D == 160) && a.Nk <= 96)
        return a.Nk > 64 && a.Nk <= 80 ? AttnKernel::ShortK80 : AttnKernel::Short;
    // two query blocks per wave where SD1.5's 4096-key level lives (d = 64 would spill: its K fragments and staging are wider)
    if (a.D == 40 && a.Nk >= 2048 && a.Nk % KT == 0) return AttnKernel::Long;
    // two query blocks per wave (attend2; d = 80 would spill 82-175 registers): halves the LDS fragment reads that bound attn_kernel;
    // worth it from 256 queries up
    if (a.D == 64 && a.Nk > 96 && a.Nq >= 256) return a.Nk >= ATTN_FAST_MIN ? AttnKernel::Q2Fast : AttnKernel::Q2;
    return a.Nk >= ATTN_FAST_MIN ? AttnKernel::Fast : AttnKernel::Exact;
}

// launch_lds for an attention kernel (arguments: a, the softmax scale, then xargs) and, once it is in the stream, the thread's launch record
// (kind, k80, qit go into the record only: a kernel that takes qit gets it once more, as its xargs)
template <auto Kern, typename T, int D, typename... X>
int launch_attn_rec(const AttnArgs& a, dim3 grid, int lds_bytes, hipStream_t s, int kind, int k80, int qit, X... xargs) {
    const int st = launch_lds<Kern>(grid, dim3(256), lds_bytes, s, a, scale_log2_of(D), xargs...);
    if (st == DSIM_OK) g_attn_last_launch = AttnLaunchRec{kind, D, sizeof(T) == 2 ? DSIM_H16 : DSIM_F32, k80, qit, (int)grid.x};
    return st;
}

// launches the tiled kernel `kind` names (every kind but P160); the `if constexpr` guards only keep kernels from being instantiated
// for a (T, D) that attention_kernel never sends to them, and such a pair returns DSIM_ERR_INVALID
template <typename T, int D>
int launch_attn_d(const AttnArgs& a, AttnKernel kind, hipStream_t s) {
    typedef ACfg<T, D> C;
    switch (kind) {
        case AttnKernel::Short:
        case AttnKernel::ShortK80:
            if constexpr (sizeof(T) == 2 && (D == 40 || D == 64 || D == 80 || D == 160)) {
                // TWO workgroups per CU whatever the K / V images need: the kernel is bound by the cache-line operations of its Q rows
                // in and O rows out, and more resident workgroups only thrash that path (64 pairs, ms at 4 | 3 | 2 | 1 workgroups per CU:
                // d = 40  0.457 | 0.426 | 0.388 | 0.447;  d = 80  0.193 | 0.181 | 0.180 | 0.191: profiles/r06_experiments.txt 4e)
                constexpr int LDSK = 96 * (C::RS + C::RSV);
                constexpr int LDSS = LDSK < 56 * 1024 ? 56 * 1024 : LDSK;
                // query blocks per workgroup: as many as keep >= 8 workgroups per CU in the grid (at most 8); the 256-register d = 160
                // instantiation (two workgroups per CU) is content with one full round.  A workgroup's blocks continue across the batch
                // elements that share its K / V.
                const int nqb = (a.Nq + 127) / 128, nvb = ((a.B + a.Bkv - 1) / a.Bkv) * nqb;
                const long want = (D > 80 ? 2L : 8L) * cu_count();
                int qit = 8;
                while (qit > 1 && (long)((nvb + qit - 1) / qit) * a.H * a.Bkv < want) qit >>= 1;
                const int nch = (nvb + qit - 1) / qit;
                const dim3 g(nch * a.H * a.Bkv);
                if (kind == AttnKernel::ShortK80) return launch_attn_rec<attn_short_kernel<D, true>, T, D>(a, g, LDSS, s, DSIM_ATTN_SHORT_K80, 1, qit, /* kernel argument: */ qit);
                return launch_attn_rec<attn_short_kernel<D, false>, T, D>(a, g, LDSS, s, DSIM_ATTN_SHORT, 0, qit, /* kernel argument: */ qit);
            }
            break;
        case AttnKernel::Long:
            if constexpr (sizeof(T) == 2 && D == 40) {
                constexpr int LDS3 = 3 * 2 * C::TILE;           // the 3-deep tile ring
                const dim3 gl(((a.Nq + 255) / 256) * a.H * a.B);
#ifdef DSIM_DEVTOOLS
                switch (g_attn_dbg) {
#define X(d) case d: return launch_attn_rec<attn_long_kernel<D, d>, T, D>(a, gl, LDS3, s, DSIM_ATTN_LONG, 0, 0);
                    X(8) X(32) X(64) X(96)
#undef X
                    default: break;
                }
#endif
                return launch_attn_rec<attn_long_kernel<D, 0>, T, D>(a, gl, LDS3, s, DSIM_ATTN_LONG, 0, 0);
            }
            break;
        case AttnKernel::Q2:
        case AttnKernel::Q2Fast:
            if constexpr (sizeof(T) == 2 && D == 64) {
                const dim3 grid2(((a.Nq + 255) / 256) * a.H * a.B);
                if (kind == AttnKernel::Q2Fast) return launch_attn_rec<attn_q2_kernel<D, true>, T, D>(a, grid2, C::LDS, s, DSIM_ATTN_Q2FAST, 0, 0);
                return launch_attn_rec<attn_q2_kernel<D, false>, T, D>(a, grid2, C::LDS, s, DSIM_ATTN_Q2, 0, 0);
            }
            break;
        case AttnKernel::Fast:
        case AttnKernel::Exact: {
            const dim3 grid(((a.Nq + 127) / 128) * a.H * a.B);
            if (kind == AttnKernel::Fast) return launch_attn_rec<attn_kernel<T, D, true>, T, D>(a, grid, C::LDS, s, DSIM_ATTN_FAST, 0, 0);
            return launch_attn_rec<attn_kernel<T, D, false>, T, D>(a, grid, C::LDS, s, DSIM_ATTN_EXACT, 0, 0);
        }
        case AttnKernel::P160:
            break;
    }
    return DSIM_ERR_INVALID;
}

template <typename T>
int launch_attn_t(const AttnArgs& a, AttnKernel kind, hipStream_t s) {
    return with_head_dim(a.D, [&](auto dc) { return launch_attn_d<T, decltype(dc)::value>(a, kind, s); });
}

}  // namespace

#ifdef DSIM_DEVTOOLS
int g_attn_dbg = 0;
#endif

inline namespace DSIM_H16_NS {
const char* attention_kernel_kind(const AttnArgs& a, int dtype) { return attn_kind_suffix((int)attention_kernel(a, dtype)); }

// the arguments launch_attention refuses whatever the kernel
static bool attention_args_ok(const AttnArgs& a, int dtype) {
    const int vec = dtype == DSIM_F32 ? 4 : 8;
    return !(a.D % 8 || a.ldq % vec || a.ldk % vec || a.ldo % 4 || a.Nk < 1 || a.Nq < 1 || a.Bkv < 1);
}

int attention_plan(const AttnArgs& a, int dtype) {
    if (!attention_args_ok(a, dtype)) return DSIM_ERR_INVALID;
    bool own = dtype == DSIM_H16;
#ifndef DSIM_H16_IS_F16
    own |= dtype == DSIM_F32;
    if (dtype == DSIM_F16) return DSIM_F16_TWIN(attention_plan(a, dtype));
#endif
    if (!own) return DSIM_ERR_INVALID;
    const int st = with_head_dim(a.D, [](auto) { return DSIM_OK; });
    return st != DSIM_OK ? st : (int)attention_kernel(a, dtype);
}

int launch_attention(const AttnArgs& a, int dtype, hipStream_t s) {
    if (!attention_args_ok(a, dtype)) return DSIM_ERR_INVALID;
    if (dtype == DSIM_H16) {
        const AttnKernel kind = attention_kernel(a, dtype);
        return kind == AttnKernel::P160 ? launch_sdpa160(a, s) : launch_attn_t<h16>(a, kind, s);
    }
#ifndef DSIM_H16_IS_F16
    if (dtype == DSIM_F32) return launch_attn_t<float>(a, attention_kernel(a, dtype), s);
    if (dtype == DSIM_F16) return DSIM_F16_TWIN(launch_attention(a, dtype, s));
#endif
    return DSIM_ERR_INVALID;
}

}  // namespace DSIM_H16_NS

}  // namespace dsim
