"""The row-resident kernels (csrc/rowres.hip: ff_fused_kernel behind op_ff_fused, rowlin_kernel behind op_ln_linear) restated twice,
shared by tests/test_rowres64_host.py, tests/test_gpu_rowres64.py and tests/test_gpu_ops.py.  Not a conftest: import it like
tests/_gemm64.py.

1. THE LATTICE FAMILY (lattice()): inputs on which the kernels' output is ONE bit pattern, whatever the order of their sums.
The kernels round at a handful of known points -- the LayerNorm's 16-bit output, hid = RN16(h * gelu_fast(g)), the epilogue's
RN16(acc2) and RN16(. + x); rowlin's RN16 of the accumulator -- and everything between them is an f32 sum of exact products of
16-bit values.  A sum whose terms are all multiples of one power of two q, with sum|terms| < 2^24 q, has every partial sum exactly
representable in f32 in every order, so the f32 result IS the real sum.  The family keeps every stage on such a grid:
  * rows x[r][c] = m_r + s_r sigma[r][c], sigma a per-row pattern of 160 entries +1 and 160 entries -1, s_r in {0.5, 1, 2}, m_r in
    {0, +-4}: the lanes' f32 sums of x are exact, the mean is m_r (1 + 2^-24-ish), the variance s_r^2 (1 + 1e-6-ish), so the
    normalised value is +-(1 - d) with d <= 2e-5 (eps = 1e-5 against s^2 = 0.25);
  * gamma in {+-0.5, +-1}, beta in {0, +-2}: fmaf(+-(1 - d), gamma, beta) lies within 2e-5 of beta +- gamma, a non-zero multiple of
    1/2 of magnitude <= 3, where half a spacing of bf16 is 2^-7 (2^-8 below 2) and of fp16 2^-10: the 16-bit LayerNorm output is
    exactly n = beta + sigma gamma.  (tests/_norm64.emulate_layernorm's rowres form reproduces it bit for bit: asserted on the CPU.)
  * W1's h rows in {0, +-1} at 25 % density, b1 multiples of 1/2: h is a multiple of 1/2.  W1's g rows hold three +-1 each (the
    first twenty rows of every 32-row chunk one in each 16-wide k-step), with a bias in {20, 24, 28}: g >= 20 - 3 x 3 = 11 by
    construction.  For g >= 8 gelu_fast(g) == g: u = min(g^2, 64) = 64, t = g (64 (64 x 1.01426306e-3 - 0.106775724) - 2.30112134)
    = -4.98 g <= -39, 1 + exp2(t) == 1 in f32 and v_rcp_f32(1) == 1 (what tests/test_gpu_norm64.ff_identity_weights() rests on).
    h g is a multiple of 1/4 below 2^22: exact in f32.  hid = RN16(h g) is a deterministic rounding of a known value;
  * W2 dense in {0, +-1/32, +-1/16}, b2 multiples of 1/16: every term of the second product is a multiple of 2^-7;
  * expected output RN16(float(RN16(acc2)) + float(x)): the epilogue's two roundings (the f32 add of two 16-bit values of these
    magnitudes is exact), computed from exact float64 values with .to(dtype);
  * the rowlin variant: the same rows and affine and a dense integer weight in {0, +-1, +-2}: RN16(n W^T), or RN16(x W^T).
lattice() asserts its own conditions (check_conditions): every g >= 8, h g exact in f32, sum|terms| 2^7 <= 2^23 for both products
(half of the exactness limit), everything finite in fp16, and that no weight the kernels read is multiplied by nothing: every
16-wide k-step of every hidden chunk has a non-zero in some h row and some g row, every k position of every hidden chunk a non-zero
in some row of each 32-row output block of W2.

2. THE FLOAT64 CHAIN AND ITS BOUND ON ORDINARY DATA (ff_ref_and_bound()).  The reference is the model's chain in float64 on the
operands as the kernel sees them (x in the compute dtype; W1, W2 rounded to it as the pack does; biases, gamma, beta f32):
y = LayerNorm(x); [h ; g] = y W1^T + b1; hid = h gelu(g) (erf form); acc2 = hid W2^T + b2; ref = acc2 + x.  u = U[dtype], U32 =
2^-24, LAM = 8 as in tests/_gemm64.py (Higham and Mary's probabilistic bound; the same Hoeffding statement serves a sum of
independent, mean-zero errors e_k with |e_k| <= a_k: |sum c_k e_k| <= LAM sqrt(sum (c_k a_k)^2) with probability >= 1 - 2 exp(-32)).
Term by term, following the kernel:
  * LayerNorm.  _norm64.ln_ref_and_bound(depth = ln_depth(rowres)) bounds the kernel's 16-bit n against y by u |y| + (1 + u) E_ln.
    Its rounding part rnd_k = u |y_k| is independent per element; the rest, com_k = (1 + u) E_ln (+ fp16's floor), is f32 error
    common to a row (the mean, the rstd) and is carried in absolute value.
      - com through W1: c1 = com @ |W1|^T, on the h and on the g rows.
      - rnd through W1: LAM sqrt(sum_k (u |y_k| w_k)^2) for one hidden value -- but the SAME 320 roundings feed all 2560 hidden
        values, so their images in different hidden units are not independent of each other and cannot be carried through W2 as if
        they were.  They are carried to the output in one step instead, through the chain's Jacobian J = W2 (diag(gelu(g)) W1h +
        diag(h gelu'(g)) W1g), gelu'(g) = Phi(g) + g phi(g): the output moves by sum_k J_ik e_k, bounded by
        LAM sqrt(sum_k (u |y_k| J_ik)^2).  (First order, as _norm64 leaves second-order terms out; J is formed in float32, a bound
        needs no more.)
  * first accumulation: LAM U32 sqrt(320) s1, s1 = |y| @ |W1|^T + |b1| (the bias is the accumulator's initial value).
  * through the GEGLU, with dh = c1_h + acc1_h, dg = c1_g + acc1_g: c_hid = |gelu(g)| dh + |h| GELU_DMAX dg + |h| GELU_FAST_ERR +
    4 U32 |hid| (gelu_fast's stated error; v_exp_f32, v_rcp_f32, the sum and the two products in f32); then the kernel's rounding of
    hid to the 16-bit type, u |hid|, independent per hidden value.
  * through W2: the independent roundings (the LayerNorm's via J, hid's via W2) share one root,
    LAM sqrt(sum_k (u |y_k| J_ik)^2 + sum_j (u |hid_j| w2_ij)^2); the rest in absolute value, (1 + u) c_hid @ |W2|^T; the second
    accumulation LAM U32 sqrt(1280) s2, s2 = |hid| @ |W2|^T + |b2|.  Their sum is E2.
  * epilogue: RN16(acc2) of the kernel's own value, u |acc2| + (1 + u) E2; the f32 add of x, U32 |ref|; the store, u |ref|:
        bound = u |ref| + (1 + u) (U32 |ref| + u |acc2| + (1 + u) E2)   (+ 2 x 2^-25 in fp16: two roundings near its subnormals).
No constant is fitted to what the kernels return.  op_ln_linear is held stage by stage instead: with the 320 x 320 identity the
kernel returns its own 16-bit LayerNorm exactly (tests/test_gpu_norm64.test_rowres_layernorm_isolated holds that to _norm64's
bound), and the dense launch is held to _gemm64.Gemm64(that tensor, w, dtype): the plain epilogue at K = 320.

replay_ff() / replay_rowlin() walk the same rounding points on the CPU (emulate_layernorm's rowres form, f32 matmuls,
_gemm64.gelu_fast64, the 16-bit roundings) and take a named mutation (MUTATIONS_FF, MUTATIONS_LIN): what a kernel bug in the weight
stream, the ring, the tile loop or the epilogue would compute.  tests/test_rowres64_host.py shows that each changes the lattice
output and which of them the float64 bound rejects."""
import math

import torch
import torch.nn.functional as F

from tests import _gemm64 as G
from tests import _norm64 as N

C = 320
HID = 4 * C
NCH = HID // 32              # hidden chunks of 32
NKS = C // 16                # k-steps of 16
NOB = C // 32                # output blocks of 32 rows of W2
TILE = 128                   # rows per workgroup tile (both kernels)
U, U32, LAM = G.U, G.U32, G.LAM
F16_MAX = 65504.0


def bits(t):
    return t.view(torch.int16)


def q16(t, dtype):
    """round to the 16-bit type, back in float64"""
    return t.to(dtype).double()


# ---- 1. the lattice family ----------------------------------------------------------------------------------------------------------
def _choice(vals, shape, gen, device="cpu"):
    v = torch.tensor(vals, dtype=torch.float64, device=device)
    return v[torch.randint(0, len(vals), shape, generator=gen, device=device)]


def lattice_weights(seed, N_lin=960):
    """the seed's weights (CPU float32, each exactly representable in bf16 and fp16): gamma, beta, w1, b1, w2, b2, wl [N_lin][320]"""
    g = torch.Generator().manual_seed(seed)
    gamma = _choice([0.5, -0.5, 1.0, -1.0], (C,), g)
    beta = _choice([0.0, 2.0, -2.0], (C,), g)
    w1 = torch.zeros(2 * HID, C, dtype=torch.float64)
    w1[:HID] = (torch.rand(HID, C, generator=g) < 0.25).double() * _choice([1.0, -1.0], (HID, C), g)
    # g rows: three +-1 each; row i of a chunk has one in k-step i (i < 20), the others anywhere
    ks = torch.randint(0, NKS, (HID, 3), generator=g)
    ks[:, 0] = torch.where(torch.arange(HID) % 32 < NKS, torch.arange(HID) % 32, ks[:, 0])
    col = 16 * ks + torch.randint(0, 16, (HID, 3), generator=g)
    sg = _choice([1.0, -1.0], (HID, 3), g)
    for j in range(3):                       # a repeated column keeps the last sign: a row may hold fewer than three
        w1[HID + torch.arange(HID), col[:, j]] = sg[:, j]
    b1 = torch.cat([torch.randint(-8, 9, (HID,), generator=g).double() / 2, _choice([20.0, 24.0, 28.0], (HID,), g)])
    w2 = torch.randint(-2, 3, (C, HID), generator=g).double() / 32
    b2 = torch.randint(-8, 9, (C,), generator=g).double() / 16
    wl = torch.randint(-2, 3, (N_lin, C), generator=g).double()
    return {k: v.float() for k, v in dict(gamma=gamma, beta=beta, w1=w1, b1=b1, w2=w2, b2=b2, wl=wl).items()}


def weight_coverage(w1, w2):
    """(h, g, w2): the family's coverage conditions, each a bool"""
    nz1 = (w1 != 0).view(2, NCH, 32, NKS, 16).any(4).any(2)                   # [half][chunk][k-step]
    nz2 = (w2 != 0).view(NOB, 32, NCH, 32).any(1)                             # [block][chunk][k position]
    return bool(nz1[0].all()), bool(nz1[1].all()), bool(nz2.all())


def lattice(M, dtype, seed, device="cpu", N_lin=960, ff=True, lin=True):
    """The exact family of (M, dtype, seed, device): weights from the seed's CPU stream, rows from `device`'s.  Returns a dict: x
    [M][320] in dtype; gamma, beta, w1, b1, w2, b2, wl f32 (on device); the expected outputs ff, lin_ln, lin (dtype; ff / lin False
    leave that operator's out) and the LayerNorm output n (dtype); cond, the quantities check_conditions() was run on.  Up to 4096
    rows the LayerNorm replay is run as well (on the CPU) and must return n."""
    w = {k: v.to(device) for k, v in lattice_weights(seed, N_lin).items()}
    g = torch.Generator(device=device).manual_seed(seed + 1)
    sigma = (torch.rand(M, C, generator=g, device=device).argsort(1) < C // 2).double() * 2 - 1
    s = _choice([0.5, 1.0, 2.0], (M, 1), g, device)
    m = _choice([0.0, 4.0, -4.0], (M, 1), g, device)
    x64 = m + s * sigma
    d = {k: v.double() for k, v in w.items()}
    n64 = d["beta"] + sigma * d["gamma"]
    t = dict(w, x=x64.to(dtype), sigma=sigma)
    assert torch.equal(t["x"].double(), x64) and torch.equal(n64.to(dtype).double(), n64)
    if M <= 4096:                                                # the kernels' LayerNorm, replayed on the CPU, returns n bit for bit
        emu = N.emulate_layernorm(t["x"], w["gamma"], w["beta"], 1e-5, dtype, dict(form="rowres"))
        assert torch.equal(bits(emu), bits(n64.to(dtype).cpu())), "the rowres LayerNorm replay does not return beta + sigma gamma"
    cond = dict(gmin=math.inf, prod_exact=True, s1=0.0, s2=0.0, sl=0.0, absmax=float(x64.abs().max()))
    a1, a2, al = d["w1"].abs(), d["w2"].abs(), d["wl"].abs()
    if ff:
        t["ff"] = torch.empty(M, C, dtype=dtype, device=device)
    if lin:
        t["lin_ln"] = torch.empty(M, N_lin, dtype=dtype, device=device)
        t["lin"] = torch.empty_like(t["lin_ln"])
    for r0 in range(0, M, 8192):
        n, xs = n64[r0:r0 + 8192], x64[r0:r0 + 8192]
        seen = []
        if ff:
            hg = n @ d["w1"].T + d["b1"]
            h, gg = hg[:, :HID], hg[:, HID:]
            prod = h * gg                                        # gelu_fast(g) == g for g >= 8
            hid = q16(prod, dtype)
            acc2 = hid @ d["w2"].T + d["b2"]
            o = q16(acc2, dtype) + xs
            t["ff"][r0:r0 + 8192] = o.to(dtype)
            cond["gmin"] = min(cond["gmin"], float(gg.min()))
            cond["prod_exact"] &= bool(torch.equal(prod.float().double(), prod))
            cond["s1"] = max(cond["s1"], float((n.abs() @ a1.T + d["b1"].abs()).max()))
            cond["s2"] = max(cond["s2"], float((hid.abs() @ a2.T + d["b2"].abs()).max()))
            seen += [hg, prod, acc2, o]
        if lin:
            yl, xl = n @ d["wl"].T, xs @ d["wl"].T
            t["lin_ln"][r0:r0 + 8192], t["lin"][r0:r0 + 8192] = yl.to(dtype), xl.to(dtype)
            cond["sl"] = max(cond["sl"], float((n.abs() @ al.T).max()), float((xs.abs() @ al.T).max()))
            seen += [yl, xl]
        cond["absmax"] = max([cond["absmax"]] + [float(v.abs().max()) for v in seen])
    cond["cover"] = weight_coverage(w["w1"].cpu(), w["w2"].cpu())
    cond["b2_nonzero"] = bool((w["b2"] != 0).any())
    check_conditions(cond)
    t.update(n=n64.to(dtype), cond=cond)
    return t


def check_conditions(c):
    assert c["gmin"] >= 8.0, c
    assert c["prod_exact"], c
    for k in ("s1", "s2", "sl"):                                 # sum|terms| in units of 2^-7: half of f32's exactness limit 2^24
        assert c[k] * 2.0 ** 7 <= 2.0 ** 23, (k, c)
    assert c["absmax"] <= F16_MAX, c
    assert c["cover"] == (True, True, True), c
    assert c["b2_nonzero"], c


def assert_bits(got, want, what=""):
    """torch.equal on the raw bits; on a mismatch the first differing (row, column), the number of differing elements and rows"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(bits(got), bits(want)):
        return
    ne = bits(got) != bits(want)
    r, c = (int(v) for v in ne.nonzero()[0])
    rows = ne.any(1)
    raise AssertionError(f"{what}: first difference at row {r} col {c} (tile {r // TILE}, wave {r % TILE // 32}): got {float(got[r, c])} "
                         f"want {float(want[r, c])}; {int(ne.sum())} elements differ in {int(rows.sum())} of {got.shape[0]} rows, "
                         f"first rows {rows.nonzero().flatten()[:8].tolist()}, columns of that row {ne[r].nonzero().flatten()[:8].tolist()}")


# ---- 2. the float64 chain and its bound ---------------------------------------------------------------------------------------------
def ff_ref_and_bound(x, gamma, beta, w1, b1, w2, b2, eps, dtype, rows=None):
    """x [M][320] in the compute dtype; gamma, beta, w1 [2560][320], b1, w2 [320][1280], b2 the f32 values the operator was given.
    rows: int64 tensor of the rows to reference (None: all).  -> (ref, bound), float64 [R][320], on x's device."""
    dev = x.device
    if rows is not None:
        x = x[rows.to(dev)]
    u = U[dtype]
    W1, W2 = G.q(w1.to(dev), dtype), G.q(w2.to(dev), dtype)
    B1, B2 = b1.to(dev).double(), b2.to(dev).double()
    A1, A2 = W1.abs(), W2.abs()
    W1h32, W1g32, W232 = W1[:HID].float(), W1[HID:].float(), W2.float()
    y, bl = N.ln_ref_and_bound(x, gamma, beta, eps, dtype, depth=N.ln_depth(dict(form="rowres"), dtype))
    rnd = u * y.abs()
    com = bl - rnd
    hg = y @ W1.T + B1
    c1 = com @ A1.T + LAM * U32 * math.sqrt(C) * (y.abs() @ A1.T + B1.abs())
    h, g = hg[:, :HID], hg[:, HID:]
    gl = F.gelu(g)
    hid = h * gl
    c_hid = gl.abs() * c1[:, :HID] + h.abs() * G.GELU_DMAX * c1[:, HID:] + h.abs() * G.GELU_FAST_ERR + 4 * U32 * hid.abs()
    acc2 = hid @ W2.T + B2
    ref = acc2 + x.double()
    dgl = 0.5 * (1 + torch.erf(g / math.sqrt(2))) + g * torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)
    ind = ((u * hid.abs()) ** 2) @ (A2 * A2).T                                  # hid's own rounding, through W2
    for r0 in range(0, x.shape[0], 32):                                        # the LayerNorm's roundings, through J (float32)
        sl = slice(r0, r0 + 32)
        T = gl[sl].float().unsqueeze(2) * W1h32 + (h[sl] * dgl[sl]).float().unsqueeze(2) * W1g32       # [r][1280][320]
        J = torch.matmul(W232, T) * rnd[sl].float().unsqueeze(1)                                       # [r][320 out][320 k]
        ind[sl] += (J.double() ** 2).sum(2)
    E2 = LAM * ind.sqrt() + (1 + u) * (c_hid @ A2.T) + LAM * U32 * math.sqrt(HID) * (hid.abs() @ A2.T + B2.abs())
    bound = u * ref.abs() + (1 + u) * (U32 * ref.abs() + u * acc2.abs() + (1 + u) * E2)
    if dtype == torch.float16:
        bound = bound + 2 * N.F16_FLOOR
    return ref, bound


def ulp(t, dtype):
    """the spacing of dtype at |t| (float64)"""
    e = torch.floor(torch.log2(t.abs().clamp_min(torch.finfo(dtype).tiny)))
    return torch.exp2(e) * torch.finfo(dtype).eps


# ---- the CPU replays and their mutations --------------------------------------------------------------------------------------------
MUT_C, MUT_KS, MUT_B = 17, 7, 4          # the hidden chunk, the k-step and the output / weight block the single-site mutations hit
MUTATIONS_FF = ("h_kstep_dropped", "g_kstep_dropped", "h_g_swapped", "chunk39_dropped", "chunk0_dropped", "w2_k_swapped",
                "w2_block_from_neighbour", "residual_from_next_row", "b2_twice", "tile1_from_tile0_rows")
MUTATIONS_LIN = ("block_reused", "k_slab_dropped")


def replay_ff(x, gamma, beta, w1, b1, w2, b2, eps, dtype, mut=None):
    """ff_fused_kernel's rounding points on the CPU -> [M][320] in dtype.  mut: one of MUTATIONS_FF."""
    assert mut is None or mut in MUTATIONS_FF
    x = x.cpu()
    w1, b1, w2, b2 = w1.cpu().to(dtype).float().clone(), b1.cpu().float().clone(), w2.cpu().to(dtype).float().clone(), b2.cpu().float().clone()
    hr, gr = slice(32 * MUT_C, 32 * MUT_C + 32), slice(HID + 32 * MUT_C, HID + 32 * MUT_C + 32)
    kr = slice(16 * MUT_KS, 16 * MUT_KS + 16)
    if mut == "h_kstep_dropped":
        w1[hr, kr] = 0
    elif mut == "g_kstep_dropped":
        w1[gr, kr] = 0
    elif mut == "h_g_swapped":
        w1[hr], w1[gr] = w1[gr].clone(), w1[hr].clone()
        b1[hr], b1[gr] = b1[gr].clone(), b1[hr].clone()
    elif mut == "chunk39_dropped":
        w2[:, 32 * 39:] = 0
    elif mut == "chunk0_dropped":
        w2[:, :32] = 0
    elif mut == "w2_k_swapped":
        a, b = 32 * MUT_C + 5, 32 * MUT_C + 22
        w2[:, a], w2[:, b] = w2[:, b].clone(), w2[:, a].clone()
    elif mut == "w2_block_from_neighbour":
        w2[32 * MUT_B:32 * MUT_B + 32] = w2[32 * MUT_B + 32:32 * MUT_B + 64].clone()
    elif mut == "b2_twice":
        b2 = 2 * b2
    n = N.emulate_layernorm(x, gamma, beta, eps, dtype, dict(form="rowres")).float()
    if mut == "tile1_from_tile0_rows":
        k = min(TILE, n.shape[0] - TILE)
        n[TILE:TILE + k] = n[:k].clone()
    hg = n @ w1.T + b1
    h, g = hg[:, :HID], hg[:, HID:]
    hid = (h * G.gelu_fast64(g.double()).float()).to(dtype).float()
    acc2 = hid @ w2.T + b2
    res = x.float().roll(-1, 0) if mut == "residual_from_next_row" else x.float()
    return (acc2.to(dtype).float() + res).to(dtype)


def replay_rowlin(x, gamma, beta, w, eps, dtype, mut=None):
    """rowlin_kernel's rounding points on the CPU (gamma = None: no LayerNorm) -> (out [M][N], the 16-bit operand [M][320]).  mut: one
    of MUTATIONS_LIN."""
    assert mut is None or mut in MUTATIONS_LIN
    x = x.cpu()
    w = w.cpu().to(dtype).float().clone()
    if mut == "block_reused":
        w[32:64] = w[:32].clone()
    elif mut == "k_slab_dropped":
        w[:, 64 * 3:64 * 4] = 0
    n = x if gamma is None else N.emulate_layernorm(x, gamma, beta, eps, dtype, dict(form="rowres"))
    return (n.float() @ w.T).to(dtype), n


def random_inputs(M, dtype, seed, N_lin=960):
    """ordinary data, as tests/test_gpu_ops.py's test_ff_fused_320 / test_ln_linear_320 draw it (CPU; x in dtype, the rest f32)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, C, generator=g) * 1.5 + 0.3).to(dtype)
    gamma, beta = torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.1
    w1 = torch.randn(2 * HID, C, generator=g) / math.sqrt(C)
    b1 = torch.randn(2 * HID, generator=g) * 0.5
    w2 = torch.randn(C, HID, generator=g) / math.sqrt(HID)
    b2 = torch.randn(C, generator=g) * 0.5
    wl = torch.randn(N_lin, C, generator=g) / math.sqrt(C)
    return dict(x=x, gamma=gamma, beta=beta, w1=w1, b1=b1, w2=w2, b2=b2, wl=wl)


def ff_args(t):
    return t["gamma"], t["beta"], t["w1"], t["b1"], t["w2"], t["b2"]
