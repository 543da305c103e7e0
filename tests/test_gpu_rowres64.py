"""The row-resident kernels (csrc/rowres.hip: ff_fused_kernel, rowlin_kernel, and the two pack kernels behind them) to the bit, and
against float64 (tests/_rowres64.py: the lattice family, the float64 chain and its bound).

Bit for bit, on the lattice family, bf16 and the fp16 twins:
  * op_ff_fused at M = 1 (a single row), 33 (rows into a second wave), 128 + 31 (two tiles, a ragged last one) and
    128 (CUs + 2) + 33 (a second tile per workgroup with a ragged end: the row prefetch and the chunk-0 prefetch across tiles); once
    more in place, out aliasing x, through dsim_op_ff_fused_dt as the executors call it; two launches bit-identical;
  * op_ln_linear with and without its LayerNorm at every N = 64, 128, ..., 960 (M = 161), and at M = 128 (3 CUs + 2) + 33 for N = 64
    (`blk` wraps every two ring steps) and N = 960: the first shapes at which a rowlin workgroup takes a second tile.
At the large M the rows are drawn on the device and the expected output is computed there in float64 (exact), conditions included.
Against float64 on ordinary data (randn rows, weights randn / sqrt(K)): op_ln_linear staged -- the identity launch returns the
kernel's own 16-bit LayerNorm, the dense launch is held to _gemm64.Gemm64 on that operand -- and op_ff_fused against the chained
bound of _rowres64.ff_ref_and_bound.  test_worst_ratios prints the largest err / bound per (operator, dtype)."""
import pytest
import torch

from tests import _gemm64 as G
from tests import _norm64 as N
from tests import _rowres64 as R

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
FF_SMALL_M = (1, 33, 128 + 31)         # the host test asserts the family's conditions for these and LIN_M (seed = M)
LIN_M = 161
LIN_NS = tuple(range(64, 961, 64))
WORST = {}                             # (operator, dtype name) -> largest err / bound (printed by test_worst_ratios)
_CACHE = {}


def _eng():
    from diffsim_amd import engine
    return engine


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ff_big_m():
    return 128 * (_cus() + 2) + 33


def lin_big_m():
    return 128 * (3 * _cus() + 2) + 33


def _lattice(M, dt, **kw):
    """small M: the CPU stream's rows (what the host test checked), moved to the device; large M: drawn and referenced on the device"""
    key = (M, dt, tuple(sorted(kw.items())))
    if key not in _CACHE:
        if M <= 4096:
            t = R.lattice(M, DT[dt], M, "cpu", **kw)
            t = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in t.items()}
        else:
            t = R.lattice(M, DT[dt], M, "cuda", **kw)
        _CACHE.clear()                  # one family at a time stays resident
        _CACHE[key] = t
    return _CACHE[key]


def _ff_in_place(eng, t, dtype):
    L = eng._lib.lib()
    x2 = t["x"].clone()
    ws = [t[k].contiguous() for k in ("gamma", "beta", "w1", "b1", "w2", "b2")]
    eng._lib.check(L.dsim_op_ff_fused_dt(x2.data_ptr(), *(w.data_ptr() for w in ws), x2.data_ptr(), x2.shape[0], R.C, 1e-5,
                                         eng._TORCH2DSIM[dtype], None), "ff in place")
    return x2


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("M", FF_SMALL_M + ("big",))
def test_ff_fused_lattice_bits(M, dt):
    eng = _eng()
    M = ff_big_m() if M == "big" else M
    t = _lattice(M, dt, lin=False)
    got = eng.op_ff_fused(t["x"], *R.ff_args(t), 1e-5)
    R.assert_bits(got, t["ff"], f"op_ff_fused M={M} {dt}")
    R.assert_bits(eng.op_ff_fused(t["x"], *R.ff_args(t), 1e-5), got, f"op_ff_fused M={M} {dt}, second launch")
    R.assert_bits(_ff_in_place(eng, t, DT[dt]), t["ff"], f"op_ff_fused in place M={M} {dt}")


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("ln", [True, False])
def test_ln_linear_lattice_bits_every_n(ln, dt):
    eng = _eng()
    t = _lattice(LIN_M, dt, ff=False)
    g, b = (t["gamma"], t["beta"]) if ln else (None, None)
    want = t["lin_ln"] if ln else t["lin"]
    for Nn in LIN_NS:
        got = eng.op_ln_linear(t["x"], g, b, t["wl"][:Nn].contiguous(), 1e-5)
        R.assert_bits(got, want[:, :Nn].contiguous(), f"op_ln_linear M={LIN_M} N={Nn} ln={ln} {dt}")


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("ln", [True, False])
@pytest.mark.parametrize("Nn", [64, 960])
def test_ln_linear_lattice_bits_second_tile_per_workgroup(Nn, ln, dt):
    eng = _eng()
    M = lin_big_m()
    assert (M + 127) // 128 > 3 * _cus()
    t = _lattice(M, dt, ff=False)
    g, b = (t["gamma"], t["beta"]) if ln else (None, None)
    w = t["wl"][:Nn].contiguous()
    got = eng.op_ln_linear(t["x"], g, b, w, 1e-5)
    R.assert_bits(got, (t["lin_ln"] if ln else t["lin"])[:, :Nn].contiguous(), f"op_ln_linear M={M} N={Nn} ln={ln} {dt}")
    R.assert_bits(eng.op_ln_linear(t["x"], g, b, w, 1e-5), got, f"op_ln_linear M={M} N={Nn} ln={ln} {dt}, second launch")


# ---- against float64 on ordinary data -----------------------------------------------------------------------------------------------
def _random(M, dt):
    return {k: v.cuda() for k, v in R.random_inputs(M, DT[dt], M).items()}


def _note(op, dt, w):
    WORST[(op, dt)] = max(WORST.get((op, dt), 0.0), w)


def lin_rows(M):
    return None if M <= 4096 else torch.unique(torch.cat([G.row_subset(M, 128), torch.arange(M - 40, M)]))


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("M,Nn", [(LIN_M, 64), (LIN_M, 320), (LIN_M, 960), ("big", 960)])
def test_ln_linear_staged_against_float64(M, Nn, dt):
    """the identity launch returns the kernel's own 16-bit LayerNorm (held to _norm64's bound here as
    test_gpu_norm64.test_rowres_layernorm_isolated holds it on its input families); the dense launch on that operand is the plain
    GEMM epilogue at K = 320"""
    eng = _eng()
    dtype = DT[dt]
    M = lin_big_m() if M == "big" else M
    t = _random(M, dt)
    operand = eng.op_ln_linear(t["x"], t["gamma"], t["beta"], torch.eye(R.C, device="cuda"), 1e-5)
    ref, bound = N.ln_ref_and_bound(t["x"], t["gamma"], t["beta"], 1e-5, dtype, depth=N.ln_depth(dict(form="rowres"), dtype))
    _note("rowlin LayerNorm", dt, N.check(operand, ref, bound, f"op_ln_linear identity M={M} {dt}"))
    del ref, bound
    w = t["wl"][:Nn].contiguous()
    got = eng.op_ln_linear(t["x"], t["gamma"], t["beta"], w, 1e-5)
    rows = lin_rows(M)
    g = G.Gemm64(operand, w, dtype, rows=rows)
    _note("op_ln_linear", dt, g.check(got if rows is None else got[rows.cuda()], f"op_ln_linear M={M} N={Nn} {dt}"))


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("M", [LIN_M, "big"])
def test_ff_fused_against_float64(M, dt):
    eng = _eng()
    dtype = DT[dt]
    M = ff_big_m() if M == "big" else M
    t = _random(M, dt)
    got = eng.op_ff_fused(t["x"], *R.ff_args(t), 1e-5)
    rows = None if M <= 4096 else G.row_subset(M, 128)
    ref, bound = R.ff_ref_and_bound(t["x"], *R.ff_args(t), 1e-5, dtype, rows=rows)
    _note("op_ff_fused", dt, N.check(got if rows is None else got[rows.cuda()], ref, bound, f"op_ff_fused M={M} {dt}"))


def test_worst_ratios():
    """prints the largest err / bound per (operator, dtype) of the float64 cases that ran in this session"""
    for k in sorted(WORST):
        print(f"worst err/bound {k[1]:4s} {k[0]:16s} {WORST[k]:.3f}")
    assert all(w <= 1.0 for w in WORST.values())
