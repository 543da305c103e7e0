"""A float64 restatement of the implicit GEMM (csrc/gemm.hip, every GemmArgs epilogue) and its per-element error bound, shared by
the GEMM tests.  Not a conftest: import it like tests/_tail64.py.

The semantics are the models': out = epi(A W^T + bias), with
  * A the A0 | A1 concatenation along K (linear), or the 3x3 conv's taps of the token-major image (k = tap * C0 + c), padding 1 on
    every side, or -- pad = 0, the VAE downsample -- F.pad(x, (0, 1, 0, 1)) then no padding (oracle/cpu_ref.py, VAE Downsample2D);
    stride 2 and the nearest 2x upsample (F.interpolate(mode="nearest")) of diffusers' Upsample2D;
  * bias2 instead of bias on the rows with odd m // rows_per_batch (SDXL's per-CFG-half time embedding);
  * act 1: F.gelu(approximate="tanh") (DiT Mlp.fc1); gate / gate2: the adaLN gate multiplies the projection before the residual
    add, gate2 on the odd m // rows_per_batch (DiT's x + gate * attn(...));
  * GEGLU: h * F.gelu(g) (erf form), [h ; g] the two halves of the weight rows (diffusers GEGLU);
  * wb_rows: row block i multiplies weight matrix i (the VAE's per-image q k^T and P v).
Operands are taken as the kernel sees them: rounded to the compute dtype with round-to-nearest-even (torch's .to()).  Everything
else is float64, on the device the tensors live on (a GPU's float64 units serve the GPU tests).

THE BOUND.  Per element, with y the pre-epilogue value (A W^T + bias) of the element's column(s):

    |got - ref| <= u_out |ref|  +  (1 + u_out) E,   E = D (u_mid |y| + (1 + u_mid) lam u32 sqrt(K) s)  +  eps_epi  +  eps_f32

  * u_out: one rounding to the output dtype (2^-24 f32, 2^-8 bf16, 2^-11 fp16): the store.  The kernel rounds ITS value, which
    differs from ref by the other terms E, so the store's error is u_out (|ref| + E): the bound is u_out |ref| + (1 + u_out) E.
    Likewise the intermediate rounding below applies to y plus its accumulation error: D (u_mid |y| + (1 + u_mid) acc).
  * lam u32 sqrt(K) s, s = (|A| @ |W|^T + |bias|)_ij: the f32 accumulation.  lam = LAM = 8 is the probabilistic bound of Higham
    and Mary (SIAM J. Sci. Comput. 41(5), 2019, Theorem 3.1): for rounding errors that are independent and mean-zero,
    |s_hat - s| <= lam sqrt(n) u sum|a_k w_k| holds with probability >= 1 - 2n exp(-lam^2 / 2); at lam = 8 and n = K <= 23040
    that is a failure probability below 6e-10 per element.  It is chosen from that statement, not fitted to the kernels.  (The
    worst-case bound would be K u32 s: sqrt(K) times looser.)
  * u_mid: the 16-bit epilogues that round an intermediate.  Every epilogue of gemm_kernel passes the tile through the wave's LDS
    slab in the OUTPUT type: the register phase (gemm.hip, "register phase: the D^T -> row-major transpose", the
    __builtin_convertvector to h16x2 before the slab store; the RES16 path's pk[i][j] conversion) rounds y to the 16-bit type
    BEFORE the tanh-GELU, the gate and the residual add of the read-back phase.  So u_mid = u_out for the 16-bit act / gate /
    residual epilogues and 0 otherwise (f32; the plain epilogue, where that rounding is the store; GEGLU, whose product is
    formed in f32 from the accumulators).
  * D: how much an error in y moves the output.  |gate| (1 without one) for plain / residual; x GELU_TANH_DMAX for the
    tanh-GELU; GEGLU: |gelu(g)| for the h column's error and |h| GELU_DMAX for the g column's (each with its own s).
  * eps_epi, the epilogue's approximations:
      - 16-bit GEGLU, gelu_fast (csrc/common.h): |error| <= GELU_FAST_ERR = 2.6e-5 absolute (its comment; checked on a grid by
        tests/test_gemm64_host.py), times |h|;
      - f32 GEGLU, erf_as (gemm.hip): Abramowitz & Stegun 7.1.26, |erf error| <= 1.5e-7, so 0.5 |g| 1.5e-7 on gelu(g), times |h|;
      - tanh-GELU in its exp form (gemm.hip, x / (1 + exp2(x (a + b x^2)))): exact algebra, the error is f32's -- v_exp_f32 and
        v_rcp_f32 are 1-ulp instructions, the folded constants carry one rounding each: TANH_EXP_REL = 8 u32 relative to |x| plus
        the exponent's own rounding, ln2 / 4 |x| |t| u32 (d/dt x / (1 + 2^t) <= |x| ln2 / 4).
  * eps_f32: the epilogue's remaining f32 operations (bias add on the conv path, the gate product, the residual add, the GEGLU
    product): 4 u32 (D |y| + |residual|).
"""
import math

import torch
import torch.nn.functional as F

U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
U32 = 2.0 ** -24
LAM = 8.0
GELU_FAST_ERR = 2.6e-5          # csrc/common.h gelu_fast
ERF_AS_ERR = 1.5e-7             # Abramowitz & Stegun 7.1.26
GELU_DMAX = 1.13                # max |d/dx x Phi(x)| = 1.1289 (at x = sqrt(2))
GELU_TANH_DMAX = 1.13           # max |d/dx| of the tanh form: 1.1289 as well (to 4 digits)
TANH_EXP_REL = 8 * U32


def q(t, dtype):
    """the operand as the kernel sees it: rounded to the compute dtype (round-to-nearest-even), then float64"""
    return t.to(dtype).double()


def conv_out_hw(H, W, stride=1, ups=0, pad=1):
    if ups:
        return 2 * H, 2 * W
    if stride == 2:
        return ((H + 1) // 2, (W + 1) // 2) if pad else (H // 2, W // 2)
    return H, W


def im2col_rows(x, rows, stride=1, ups=0, pad=1):
    """A(m, k) of the 3x3 conv for the output rows `rows` (int64 tensor): x [B][H][W][C] float64 -> [len(rows)][9 C], k = tap C + c
    with tap = 3 ky + kx.  ups: the nearest 2x upsample first; pad 1: zero padding on every side; pad 0: F.pad(x, (0, 1, 0, 1))."""
    if ups:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    B, H, W, C = x.shape
    Ho, Wo = conv_out_hw(H, W, stride, 0, pad) if not ups else (H, W)
    rows = rows.to(x.device)
    b, rem = rows // (Ho * Wo), rows % (Ho * Wo)
    oy, ox = rem // Wo, rem % Wo
    off = 1 if pad else 0
    cols = []
    for ky in range(3):
        for kx in range(3):
            iy, ix = oy * stride + ky - off, ox * stride + kx - off
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            v = x[b, iy.clamp(0, H - 1), ix.clamp(0, W - 1)]
            cols.append(v * ok.unsqueeze(1).to(v.dtype))
    return torch.cat(cols, dim=1)


def conv_weight_rows(w):
    """diffusers [N][C][3][3] -> [N][9 C] in the k = tap C + c order"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def row_subset(M, tile_rows, boundaries=(), n_random=64, seed=0):
    """Rows to reference when the whole problem is too large: the first and last row of every tile_rows-row M tile, the rows on each
    side of every boundary (image starts, rows_per_batch multiples), and a seeded random sample.  Sorted int64 tensor."""
    t = torch.arange(0, M, tile_rows)
    sel = [t, (t + tile_rows - 1).clamp(max=M - 1)]
    for b in boundaries:
        sel.append(torch.tensor([b - 1, b], dtype=torch.int64))
    g = torch.Generator().manual_seed(seed)
    sel.append(torch.randint(0, M, (n_random,), generator=g))
    r = torch.cat(sel)
    return torch.unique(r[(r >= 0) & (r < M)])


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_fast64(x):
    """csrc/common.h gelu_fast in float64 with exact exp2 / reciprocal (what its documented error bound is about)"""
    u = torch.clamp(x * x, max=64.0)
    t = x * (u * (u * 1.01426306e-3 - 0.106775724) - 2.30112134)
    return x / (1.0 + torch.exp2(t))


class Gemm64:
    """The reference and bound of one GEMM launch over the output rows `rows` (None: all M).

    a0, a1, residual: tensors in the compute dtype (their values are the operands); w, bias, bias2, gate, gate2: the f32 values the
    operator was given (w rounded here as the pack does).  conv: None or dict(stride, ups, pad); epi "none" / "residual" / "geglu".
    Attributes: rows, ref [R][ncol], bound [R][ncol] (float64), y [R][N] the pre-epilogue values."""

    def __init__(self, a0, w, dtype, *, a1=None, conv=None, bias=None, bias2=None, rows_per_batch=0, act=0, gate=None, gate2=None,
                 epi="none", residual=None, wb_rows=0, rows=None, device=None):
        dev = device or a0.device
        self.dtype = dtype
        if conv is None:
            M = a0.shape[0]
            rows = torch.arange(M) if rows is None else rows
            rd = rows.to(a0.device)
            A = q(a0[rd], dtype) if a1 is None else torch.cat([q(a0[rd], dtype), q(a1[rd], dtype)], 1)
            A = A.to(dev)
            Wm = q(w.to(dev), dtype)
        else:
            B, H, W, C0 = a0.shape
            Ho, Wo = conv_out_hw(H, W, conv.get("stride", 1), conv.get("ups", 0), conv.get("pad", 1))
            M = B * Ho * Wo
            rows = torch.arange(M) if rows is None else rows
            A = im2col_rows(q(a0.to(dev), dtype), rows, conv.get("stride", 1), conv.get("ups", 0), conv.get("pad", 1))
            Wm = conv_weight_rows(q(w.to(dev), dtype))
        rows_d = rows.to(dev)
        self.rows, self.M, self.K = rows, M, A.shape[1]
        if wb_rows:
            blk = rows_d // wb_rows
            y = A.new_empty(A.shape[0], Wm.shape[1])
            s = torch.empty_like(y)
            for i in torch.unique(blk).tolist():
                sel = blk == i
                y[sel], s[sel] = A[sel] @ Wm[i].T, A[sel].abs() @ Wm[i].abs().T
        else:
            y, s = A @ Wm.T, A.abs() @ Wm.abs().T
        odd = ((rows_d // rows_per_batch) % 2 == 1).unsqueeze(1) if rows_per_batch else None
        if bias is not None:
            bv = bias.to(dev).double().unsqueeze(0)
            if bias2 is not None:
                bv = torch.where(odd, bias2.to(dev).double().unsqueeze(0), bv)
            y = y + bv
            s = s + bv.abs()
        self.y = y
        u_out = U[dtype]
        acc = LAM * U32 * math.sqrt(self.K) * s
        res = q(residual.reshape(M, -1)[rows_d.to(residual.device)], dtype).to(dev) if residual is not None else None
        if epi == "geglu":
            n2 = y.shape[1] // 2
            h, g = y[:, :n2], y[:, n2:]
            gl = F.gelu(g)
            ref = h * gl
            d_h, d_g = acc[:, :n2], acc[:, n2:]
            eps = h.abs() * (GELU_FAST_ERR if dtype != torch.float32 else 0.5 * g.abs() * ERF_AS_ERR)
            bound = gl.abs() * d_h + h.abs() * GELU_DMAX * d_g + eps + 4 * U32 * ref.abs()
        else:
            z, dz, eps = y, torch.ones_like(y), torch.zeros_like(y)
            if act == 1:
                z = gelu_tanh64(y)
                dz = dz * GELU_TANH_DMAX
                t = y * (-0.10294324 * y * y - 2.3022082)
                eps = TANH_EXP_REL * y.abs() + math.log(2) / 4 * y.abs() * t.abs() * U32
            if gate is not None:
                gv = gate.to(dev).double().unsqueeze(0)
                if gate2 is not None:
                    gv = torch.where(odd, gate2.to(dev).double().unsqueeze(0), gv)
                z, dz, eps = z * gv, dz * gv.abs(), eps * gv.abs()
            if res is not None:
                z = z + res[:, : z.shape[1]]
            ref = z
            mid = u_out if (dtype != torch.float32 and (act or gate is not None or res is not None)) else 0.0
            bound = dz * (mid * y.abs() + (1 + mid) * acc) + eps + 4 * U32 * (dz * y.abs() + (res[:, : z.shape[1]].abs() if res is not None else 0))
        self.ref = ref
        self.bound = u_out * ref.abs() + (1 + u_out) * bound

    def check(self, got, what=""):
        """got: the kernel's [R][ncol] rows (any dtype / device).  Returns the largest err / bound; raises on any violation."""
        g = got.to(self.ref.device).double()
        assert torch.isfinite(g).all(), f"{what}: non-finite output"
        err = (g - self.ref).abs()
        ratio = err / self.bound.clamp_min(1e-300)
        worst = float(ratio.max())
        if worst > 1.0:
            i = int(ratio.argmax())
            r, c = divmod(i, ratio.shape[1])
            raise AssertionError(f"{what}: {int((ratio > 1).sum())} elements out of bound; worst row {int(self.rows[r])} col {c}: "
                                 f"got {float(g[r, c]):.6g} ref {float(self.ref[r, c]):.6g} bound {float(self.bound[r, c]):.3g}")
        return worst
