"""Inputs for tests/test_gpu_rowlin_forms.py: the row-resident Linear's forms beyond K = 320 behind a LayerNorm (csrc/rowres.hip:
rowlin640_kernel, gn_rowlin_kernel).  Not a conftest: import it like tests/_rowres64.py, whose lattice family this extends.

lattice(M, C, ...) is _rowres64.lattice()'s rowlin variant at any even width C (C = 640 here): rows x[r][c] = m_r + s_r sigma[r][c]
with sigma a per-row pattern of C / 2 entries +1 and C / 2 entries -1, s_r in {0.5, 1, 2}, m_r in {0, +-4}; gamma in {+-0.5, +-1},
beta in {0, +-2}; a dense integer weight in {0, +-1, +-2}.  The 16-bit LayerNorm output is exactly n = beta + sigma gamma (the rowres
LayerNorm replay of tests/_norm64.py returns it bit for bit: asserted on the CPU for M <= 4096), every term of either product is a
multiple of 1/2 and sum|terms| <= 6 x 2 x 640 = 7680 < 2^16: every partial sum is exact in f32 in every order, so the kernel's output
is ONE bit pattern, RN16(n W^T) or RN16(x W^T).  The conditions are asserted here, on the tensors drawn."""
import math

import torch

from tests import _norm64 as N
from tests import _rowres64 as R


def lattice_weights(seed, C, N_lin):
    g = torch.Generator().manual_seed(seed)
    gamma = R._choice([0.5, -0.5, 1.0, -1.0], (C,), g)
    beta = R._choice([0.0, 2.0, -2.0], (C,), g)
    wl = torch.randint(-2, 3, (N_lin, C), generator=g).double()
    return {k: v.float() for k, v in dict(gamma=gamma, beta=beta, wl=wl).items()}


def lattice(M, C, dtype, seed, device="cpu", N_lin=1920):
    """-> dict: x [M][C] in dtype; gamma, beta, wl [N_lin][C] f32; lin_ln, lin [M][N_lin] in dtype: the expected outputs with and
    without the LayerNorm"""
    w = {k: v.to(device) for k, v in lattice_weights(seed, C, N_lin).items()}
    g = torch.Generator(device=device).manual_seed(seed + 1)
    sigma = (torch.rand(M, C, generator=g, device=device).argsort(1) < C // 2).double() * 2 - 1
    s = R._choice([0.5, 1.0, 2.0], (M, 1), g, device)
    m = R._choice([0.0, 4.0, -4.0], (M, 1), g, device)
    x64 = m + s * sigma
    d = {k: v.double() for k, v in w.items()}
    n64 = d["beta"] + sigma * d["gamma"]
    t = dict(w, x=x64.to(dtype))
    assert torch.equal(t["x"].double(), x64) and torch.equal(n64.to(dtype).double(), n64)
    if M <= 4096:
        emu = N.emulate_layernorm(t["x"], w["gamma"], w["beta"], 1e-5, dtype, dict(form="rowres"))
        assert torch.equal(R.bits(emu), R.bits(n64.to(dtype).cpu())), "the rowres LayerNorm replay does not return beta + sigma gamma"
    t["lin_ln"] = torch.empty(M, N_lin, dtype=dtype, device=device)
    t["lin"] = torch.empty_like(t["lin_ln"])
    al = d["wl"].abs()
    sl = absmax = 0.0
    for r0 in range(0, M, 8192):
        n, xs = n64[r0:r0 + 8192], x64[r0:r0 + 8192]
        yl, xl = n @ d["wl"].T, xs @ d["wl"].T
        t["lin_ln"][r0:r0 + 8192], t["lin"][r0:r0 + 8192] = yl.to(dtype), xl.to(dtype)
        sl = max(sl, float((n.abs() @ al.T).max()), float((xs.abs() @ al.T).max()))
        absmax = max(absmax, float(yl.abs().max()), float(xl.abs().max()))
    assert sl * 2.0 ** 7 <= 2.0 ** 23, sl                        # sum|terms| in units of 2^-7: half of f32's exactness limit
    assert absmax <= R.F16_MAX, absmax
    # no weight is multiplied by nothing: every 16-wide k-step of every 32-row block holds a non-zero
    assert bool((w["wl"].cpu() != 0).view(N_lin // 32, 32, C // 16, 16).any(3).any(1).all())
    return t


def random_ln_inputs(M, C, dtype, seed, N_lin):
    """ordinary data, as _rowres64.random_inputs draws it; every fifth row (and row 0) carries a mean far above its spread"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g) * 1.5 + 0.3
    x[::5] += 60.0
    gamma, beta = torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.1
    wl = torch.randn(N_lin, C, generator=g) / math.sqrt(C)
    return dict(x=x.to(dtype), gamma=gamma, beta=beta, wl=wl)


def random_gn_inputs(B, HW, C, dtype, seed):
    """x [B][HW][C] randn; image 1 (the only image of B = 1) carries per-channel offsets far above its spread; gamma, beta, w [C][C],
    bias f32"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, HW, C, generator=g) * 1.5 + 0.3
    x[min(1, B - 1)] += (torch.randn(C, generator=g) * 10.0 + 50.0).view(1, C)
    gamma, beta = torch.randn(C, generator=g) * 0.2 + 1.0, torch.randn(C, generator=g) * 0.1
    w = torch.randn(C, C, generator=g) / math.sqrt(C)
    bias = torch.randn(C, generator=g) * 0.5
    return dict(x=x.to(dtype), gamma=gamma, beta=beta, w=w, bias=bias)
