"""tests/_front64.py checked where no GPU is needed: each float64 restatement against torch's own float64 operator, the integer
restatement of the nearest resize against F.interpolate, the derived bounds against a float32 replay of each arithmetic kernel on
the GPU test's own case list (the REFERENCE SIDE ALONE must sit inside the bound; the worst err / bound per operator is printed), and
the header / binding parity of the new entry points."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import _front64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dsim_op_conv_in", "dsim_op_timestep_sincos", "dsim_op_sincos_values", "dsim_op_gemv_f32", "dsim_op_pack",
               "dsim_op_dup_batch", "dsim_op_resize_nearest", "dsim_op_gather_ctx", "dsim_op_patch_embed", "dsim_op_fold_quant",
               "dsim_op_to_nchw_f32")


def test_abi_parity_of_the_new_entry_points():
    from diffsim_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    assert re.search(r"#define\s+DSIM_ABI_VERSION\s+7\b", hdr) and _lib.ABI_VERSION == 7        # additive: the version stays
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_SYMBOLS:
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared in the header"
        assert name in _lib.SYMBOLS, f"{name} has no binding"
        assert len(_lib.SYMBOLS[name][1]) == len(m.group(1).split(",")), f"{name}: the binding's argument count differs from the header's"
    # the enums the bindings index by value
    assert re.search(r"DSIM_CONV_IN_GENERIC\s*=\s*1,.*DSIM_CONV_IN_EIGHT\s*=\s*2,.*DSIM_CONV_IN_ROWS\s*=\s*3", code, flags=re.S)
    assert _lib.CONV_IN_KERNELS == (None, "generic", "eight", "rows")
    assert re.search(r"DSIM_PACK_LINEAR\s*=\s*0,\s*DSIM_PACK_CONV3\s*=\s*1,\s*DSIM_PACK_CONV_IN\s*=\s*2,\s*DSIM_PACK_VECTOR\s*=\s*3", code)
    assert _lib.PACK_KINDS == ("linear", "conv3", "conv_in", "vector")


# ---- the restatements against torch's own float64 operators -----------------------------------------------------------------------
@pytest.mark.parametrize("noise", [True, False])
@pytest.mark.parametrize("dup", [1, 2])
def test_conv_in_restatement_is_conv2d(noise, dup):
    lat, nz, sa, sb, w, b = R.conv_in_inputs(4, 7, 24, 3)
    ref, _ = R.conv_in_ref_and_bound(lat, nz if noise else None, sa, sb, w, b, torch.float32, dup)
    x = (float(torch.tensor(sa)) * lat.double() + float(torch.tensor(sb)) * nz.double()) if noise else lat.double()
    y = F.conv2d(x, w.double(), b.double(), padding=1)                                  # [n][Cout][S][S]
    want = torch.cat([y, y], 0) if dup == 2 else y                                      # diffusers' CFG duplication: cat([x] * 2)
    want = want.flatten(2).transpose(1, 2)
    # the engine keeps the copies of one image together ([img * dup + d]); torch.cat puts copy d of image i at d * n + i
    order = torch.tensor([d * 3 + i for i in range(3) for d in range(dup)])
    assert torch.allclose(ref, want[order], rtol=0, atol=1e-13)
    rows = torch.tensor([0, 3, 6])
    sub, sb_ = R.conv_in_ref_and_bound(lat, nz if noise else None, sa, sb, w, b, torch.float32, dup, rows=rows)
    full, fb = R.conv_in_ref_and_bound(lat, nz if noise else None, sa, sb, w, b, torch.float32, dup)
    pick = (rows.view(-1, 1) * 7 + torch.arange(7).view(1, -1)).flatten()
    assert torch.allclose(sub, full[:, pick], rtol=0, atol=1e-13) and torch.allclose(sb_, fb[:, pick], rtol=1e-9, atol=0)


def test_patch_restatement_is_a_reshape_projection():
    for Cin, S, p, D in ((4, 10, 2, 24), (3, 8, 4, 16)):
        lat, nz, sa, sb, w, b, pos = R.patch_inputs(Cin, S, p, D, 2)
        ref, _ = R.patch_ref_and_bound(lat, nz, sa, sb, w, b, pos, p, torch.float32)
        x = float(torch.tensor(sa)) * lat.double() + float(torch.tensor(sb)) * nz.double()
        g = S // p
        tok = x.view(2, Cin, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(2, g * g, Cin * p * p)       # k = (c p + py) p + px
        want = tok @ w.double().view(D, -1).T + b.double() + pos.double()
        assert torch.allclose(ref[0::2], want, rtol=0, atol=1e-13) and torch.equal(ref[0::2], ref[1::2])


def test_sincos_restatement_is_diffusers_timesteps():
    for dim in R.SINCOS_DIMS:
        half = dim // 2
        ts = torch.tensor(R.SINCOS_T, dtype=torch.float64)
        exponent = -math.log(10000) * torch.arange(half, dtype=torch.float64) / (half - 0.0)          # downscale_freq_shift = 0
        emb = ts[:, None] * torch.exp(exponent)[None, :]
        emb = torch.cat([torch.sin(emb), torch.cos(emb)], -1)
        emb = torch.cat([emb[:, half:], emb[:, :half]], -1)                                            # flip_sin_to_cos
        ref, _ = R.sincos_ref_and_bound(dim, [float(t) for t in R.SINCOS_T])
        assert torch.allclose(ref, emb, rtol=0, atol=1e-13)


def test_gemv_restatement_is_linear_of_silu():
    W, b, x = R.gemv_inputs(5, 65, torch.float32, torch.float32)
    for act in (0, 1):
        ref, _ = R.gemv_ref_and_bound(W, b, x, act)
        want = F.linear(F.silu(x.double()) if act else x.double(), W.double(), b.double())
        assert torch.allclose(ref, want, rtol=1e-13, atol=1e-13)


def test_resize_restatement_is_interpolate_nearest():
    for n_in in range(1, 41):
        for n_out in {2 * n_in - 1, 2 * n_in, 2 * n_in + 1, n_in // 2, n_in + 3}:
            if n_out < 1:
                continue
            x = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
            want = F.interpolate(x, size=(n_out, 1), mode="nearest").flatten().long()
            assert torch.equal(R.nearest_index(n_in, n_out), want), (n_in, n_out)
    x = torch.randn(2, 13, 7, 8)
    assert torch.equal(R.resize_ref(x, 25, 13), R.resize_ref_torch(x, 25, 13))


def test_exact_restatements():
    # the GEGLU interleave: packed blocks alternate h and g blocks of the source, in order
    for N, rows in ((64, 32), (640, 16), (2560, 32)):
        s = R.geglu_src_rows(N, rows).view(-1, rows)
        assert torch.equal(s.flatten().sort().values, torch.arange(N))
        for b in range(s.shape[0]):
            first = (b // 2) * rows + (N // 2 if b % 2 else 0)
            assert torch.equal(s[b], torch.arange(first, first + rows))
    w = torch.randn(5, 3, 3, 3)
    p3, pin = R.pack_ref("conv3", w, torch.float32), R.pack_ref("conv_in", w, torch.float32)
    for co, ci, ky, kx in ((0, 0, 0, 0), (4, 2, 1, 2), (3, 1, 2, 0)):
        assert p3[co, ky * 3 + kx, ci] == w[co, ci, ky, kx] and pin[(ky * 3 + kx) * 3 + ci, co] == w[co, ci, ky, kx]
    ctx = torch.randn(3, 2, 5)
    got = R.gather_ref(ctx, torch.tensor([2, -1, 3, 2 ** 30, 0], dtype=torch.int32), torch.float32)
    assert torch.equal(got.view(5, 2, 5), ctx[[2, 0, 2, 2, 0]])
    x = torch.randn(2, 25, 8)
    assert torch.equal(R.nchw_ref(x), x.view(2, 5, 5, 8).permute(0, 3, 1, 2).reshape(2, 8, 25))
    assert torch.equal(R.dup_ref(torch.arange(3))[:, None].flatten(), torch.tensor([0, 0, 1, 1, 2, 2]))


# ---- the bounds hold for the reference arithmetic alone, on the GPU test's case list ----------------------------------------------
WORST = {}


def _note(op, w):
    WORST[op] = max(WORST.get(op, 0.0), w)


@pytest.mark.parametrize("dt", list(R.DT))
def test_conv_in_bound_holds_for_a_float32_replay(dt):
    dtype = R.DT[dt]
    for (Cin, S, Cout) in R.CONV_IN_CASES:
        for noise in (True, False):
            lat, nz, sa, sb, w, b = R.conv_in_inputs(Cin, S, Cout, 1)
            nz = nz if noise else None
            ref, bound = R.conv_in_ref_and_bound(lat, nz, sa, sb, w, b, dtype)
            _note(f"conv_in {dt}", R.check(R.emulate_conv_in(lat, nz, sa, sb, w, b, dtype), ref, bound, f"conv_in {Cin} {S} {Cout} {dt}"))


@pytest.mark.parametrize("dt", list(R.DT))
def test_patch_bound_holds_for_a_float32_replay(dt):
    dtype = R.DT[dt]
    for (Cin, S, p, D) in R.PATCH_CASES:
        t = R.patch_inputs(Cin, S, p, D, 1)
        ref, bound = R.patch_ref_and_bound(*t, p, dtype)
        _note(f"patch_embed {dt}", R.check(R.emulate_patch_embed(*t, p, dtype), ref, bound, f"patch {Cin} {S} {p} {D} {dt}"))


def test_sincos_bound_holds_for_a_float32_replay():
    for dim in R.SINCOS_DIMS:
        for vals in ([float(t) for t in R.SINCOS_T],) + tuple(R.SINCOS_VALUES.values()):
            v32 = torch.tensor(vals, dtype=torch.float32)
            ref, bound = R.sincos_ref_and_bound(dim, v32)
            _note("sincos f32", R.check(R.emulate_sincos(dim, v32), ref, bound, f"sincos {dim}"))


def test_gemv_bound_holds_for_a_float32_replay():
    for (N, K) in R.GEMV_SHAPES:
        for wdt, bdt, act in ((torch.float32, torch.float32, 1), (torch.bfloat16, None, 0), (torch.float16, torch.float16, 1)):
            W, b, x = R.gemv_inputs(N, K, wdt, bdt)
            ref, bound = R.gemv_ref_and_bound(W, b, x, act)
            _note("gemv f32", R.check(R.emulate_gemv(W, b, x, act), ref, bound, f"gemv {N} {K} {wdt} act {act}"))


@pytest.mark.parametrize("dt", list(R.DT))
def test_fold_bound_holds_for_a_float32_replay(dt):
    dtype = R.DT[dt]
    for (Cm, K) in R.FOLD_CASES:
        wq, wco, bco, bq = R.fold_inputs(Cm, K, dtype)
        ref, bound = R.fold_ref_and_bound(wq, wco, dtype)
        _note(f"fold_quant {dt}", R.check(R.emulate_fold(wq, wco, dtype), ref, bound, f"fold {Cm} {K} {dt}"))
        ref, bound = R.fold_bias_ref_and_bound(wq, bco, bq)
        _note("fold_quant bias", R.check(R.emulate_fold_bias(wq, bco, bq), ref, bound, f"fold bias {Cm}"))


def test_print_worst_ratios():
    """(runs last in this file) the worst err / bound of the float32 replays, per operator"""
    for k in sorted(WORST):
        print(f"replay worst err/bound {k:20s} {WORST[k]:.3f}")
    assert all(w <= 1.0 for w in WORST.values())
