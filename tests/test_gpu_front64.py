"""The kernels in front of the models against float64, element by element (tests/_front64.py: the references and their derived
bounds): noising + conv_in in its three kernels, the GroupNorm partials of the VAE's row kernel, the sinusoidal embeddings, the
time-embedding GEMV, the four weight packs from every checkpoint dtype, dup_batch / resize_nearest / gather_ctx, DiT's patch embedding,
the VAE's quant_conv fold and its output transpose.  Each runs through its single-operator entry point (dsim_op_*) on a buffer the test
owns, in bf16, fp16 and f32 wherever the kernel is typed.  Every arithmetic case checks, on EVERY element,
  * the bound, and that the output is finite;
  * a sentinel-filled output with guards before and after it: nothing left unwritten inside, nothing touched outside;
  * two runs bit-identical.
The exact operators (packs, transposes, copies, gathers, the resize) are compared with torch.equal on the same guarded buffers.
conv_in additionally holds the kernel each shape reports to the table in tests/_front64.py CONV_IN_CASES (the launch coverage of the
family), the CFG copies to bit equality in [img * dup + d] order, and the three kernels to the bit identity their comments claim.
test_worst_ratios prints the worst err / bound per (operator, dtype)."""
import math

import pytest
import torch

from tests import _front64 as R

pytestmark = pytest.mark.gpu

DT = R.DT
SENT = -12345.0              # fill of the output buffer: what the kernel must overwrite inside and leave alone outside
WORST = {}                   # (operator, dtype name) -> largest err / bound


def _eng():
    from diffsim_amd import engine
    return engine


def _invalid(fn):
    from diffsim_amd import _lib
    with pytest.raises(_lib.DsimError, match="invalid argument"):
        fn()


def _note(op, dt, w):
    WORST[(op, dt)] = max(WORST.get((op, dt), 0.0), w)


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.int8}[t.element_size()])


def _run(fn, shape, dtype):
    """fn(out) on a sentinel-filled buffer with guards of at least four rows before and after `shape` elements; asserts the guards
    untouched and nothing inside left unwritten.  -> (the written tensor [shape], whatever fn returned)"""
    n = math.prod(shape)
    g = -(-max(64, 4 * shape[-1]) // 8) * 8                                # (a multiple of 16 bytes: the kernels store 16-byte vectors)
    buf = torch.full((n + 2 * g,), SENT, dtype=dtype, device="cuda")
    out = buf[g:g + n]
    r = fn(out)
    torch.cuda.synchronize()
    sent = torch.tensor(SENT, dtype=dtype, device="cuda")
    assert (buf[:g] == sent).all() and (buf[g + n:] == sent).all(), "written outside the output"
    assert not (out == sent).any(), "output elements left unwritten"
    return out.view(shape), r


def _cuda(*ts):
    return [t.cuda() if torch.is_tensor(t) else t for t in ts]


# ---- conv_in ---------------------------------------------------------------------------------------------------------------------
def _conv_in_once(t, dtype, dup, force=0, rows=None, gn_part=None):
    lat, nz, sa, sb, w, b = t
    n, _, S, _ = lat.shape
    shape = (n * dup, S * S, w.shape[0])
    return _run(lambda o: _eng().op_conv_in(lat, nz, sa, sb, w, b, dtype, dup=dup, force=force, gn_part=gn_part, out=o)[1], shape, dtype)


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("case", list(R.CONV_IN_CASES), ids=lambda c: "x".join(map(str, c)))
def test_conv_in_against_float64(case, dt):
    dtype = DT[dt]
    Cin, S, Cout = case
    for n_img in (1, 3):
        host = R.conv_in_inputs(Cin, S, Cout, n_img)
        lat, nz, sa, sb, w, b = _cuda(*host)
        for noised in (True, False):
            for dup in (1, 2):
                t = (lat, nz if noised else None, sa, sb, w, b)
                what = f"conv_in {case} n {n_img} noise {noised} dup {dup} {dt}"
                got, kern = _conv_in_once(t, dtype, dup)
                assert kern == R.CONV_IN_CASES[case], (what, kern)
                ref, bound = R.conv_in_ref_and_bound(host[0], host[1] if noised else None, *host[2:], dtype, dup)
                _note(f"conv_in_{kern}", dt, R.check(got, ref, bound, what))
                if dup == 2:
                    v = got.view(n_img, 2, S * S, Cout)
                    assert torch.equal(_bits(v[:, 0]), _bits(v[:, 1])), f"{what}: the CFG copies differ"
                assert torch.equal(_bits(_conv_in_once(t, dtype, dup)[0]), _bits(got)), f"{what}: two runs differ"


@pytest.mark.parametrize("dt", list(DT))
def test_conv_in_kernels_are_bit_identical(dt):
    """the comments of prep_conv_in8_kernel and conv_in_rows_kernel: the same bias-first ascending-k fmaf chain as prep_conv_in_kernel"""
    dtype = DT[dt]
    lat, nz, sa, sb, w, b = _cuda(*R.conv_in_inputs(3, 64, 128, 2))
    outs = {}
    for force, name in ((1, "generic"), (2, "eight"), (3, "rows")):
        outs[name], kern = _conv_in_once((lat, None, sa, sb, w, b), dtype, 1, force=force)
        assert kern == name
    assert torch.equal(_bits(outs["generic"]), _bits(outs["eight"])), "eight-wide differs from generic at 3 x 64 -> 128"
    assert torch.equal(_bits(outs["generic"]), _bits(outs["rows"])), "row kernel differs from generic at 3 x 64 -> 128"
    t = tuple(_cuda(*R.conv_in_inputs(4, 8, 320, 3)))
    a, ka = _conv_in_once(t, dtype, 2, force=1)
    e, ke = _conv_in_once(t, dtype, 2, force=2)
    assert (ka, ke) == ("generic", "eight") and torch.equal(_bits(a), _bits(e)), "eight-wide differs from generic at 4 x 8 -> 320"


def test_conv_in_refuses_a_forced_kernel_that_does_not_apply():
    E = _eng()
    for (Cin, S, Cout), force, noise in (((4, 9, 100), 2, True),          # Cout % 8 != 0
                                         ((4, 9, 8), 2, True),            # 1024 pixels x 36 f32 of staging: over 48 KB
                                         ((4, 8, 320), 3, False),         # not the VAE's shape
                                         ((3, 64, 128), 3, True),         # the row kernel does not noise
                                         ((3, 48, 128), 3, False)):       # S % 64 != 0
        lat, nz, sa, sb, w, b = _cuda(*R.conv_in_inputs(Cin, S, Cout, 1))
        _invalid(lambda: E.op_conv_in(lat, nz if noise else None, sa, sb, w, b, torch.bfloat16, force=force))
    lat, nz, sa, sb, w, b = _cuda(*R.conv_in_inputs(3, 64, 128, 1))
    part = torch.zeros(1, 64, 32, 2, device="cuda")
    _invalid(lambda: E.op_conv_in(lat, None, sa, sb, w, b, torch.float32, gn_part=part))                 # statistics are 16-bit only
    _invalid(lambda: E.op_conv_in(lat, None, sa, sb, w, b, torch.bfloat16, force=2, gn_part=part))       # ... and the row kernel's
    _invalid(lambda: E.op_conv_in(lat, None, sa, sb, w, b, torch.bfloat16, force=4))
    _invalid(lambda: E.op_conv_in(lat, None, sa, sb, w, b, torch.bfloat16, dup=3))


def _check_partials(got, part, n, S, dtype, name):
    """tests/test_gpu_gemm64.py's _check_gn on the row kernel's partials: every slot written, the 256-term bound on the sums of the
    STORED values, and op_groupnorm_pre on them within tests/_norm64.py's bound of float64 GroupNorm + SiLU"""
    from tests import test_gpu_gemm64 as TG
    TG.CASES[name] = dict(B=n)
    try:
        TG._check_gn(name, dict(N=128, dtype=dtype), got.reshape(n * S * S, 128), dict(gn_hw=S * S, gn_part=part))
    finally:
        del TG.CASES[name]


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("S,n_img", [(64, 2), (128, 1), (192, 1), (256, 1)])
def test_conv_in_rows_against_float64(S, n_img, dt):
    """S / 64 = 1, 2, 3, 4 segments per image row: a workgroup walks nseg = 1, 2, 1, 4 of them (4: both LDS buffers reused)"""
    dtype = DT[dt]
    host = R.conv_in_inputs(3, S, 128, n_img)
    lat, _, sa, sb, w, b = _cuda(*host)
    t = (lat, None, sa, sb, w, b)
    part = None if dt == "f32" else torch.full((n_img, S * S // 64, 32, 2), float("nan"), device="cuda")
    got, kern = _conv_in_once(t, dtype, 1, gn_part=part)
    assert kern == "rows"
    ref, bound = R.conv_in_ref_and_bound(host[0], None, *host[2:], dtype)
    _note("conv_in_rows", dt, R.check(got, ref, bound, f"conv_in_rows S {S} {dt}"))
    del ref, bound
    if part is not None:
        _check_partials(got, part, n_img, S, dtype, f"front64_rows_{S}_{dt}")
        plain, _ = _conv_in_once(t, dtype, 1)
        assert torch.equal(_bits(plain), _bits(got)), "the statistics epilogue changes the stored values"
        part2 = torch.full_like(part, float("nan"))
        again, _ = _conv_in_once(t, dtype, 1, gn_part=part2)
        assert torch.equal(_bits(again), _bits(got)) and torch.equal(_bits(part2), _bits(part)), "two runs differ"
    else:
        assert torch.equal(_bits(_conv_in_once(t, dtype, 1)[0]), _bits(got)), "two runs differ"


@pytest.mark.parametrize("dt", list(DT))
def test_conv_in_rows_512(dt):
    """the VAE's own size, two images: eight segments per workgroup.  Referenced on the first and last image rows and the rows either
    side of the middle, each whole (the first and the last segment of a workgroup's walk included); written / guards on everything."""
    dtype, S, n = DT[dt], 512, 2
    host = R.conv_in_inputs(3, S, 128, n)
    lat, _, sa, sb, w, b = _cuda(*host)
    part = None if dt == "f32" else torch.full((n, S * S // 64, 32, 2), float("nan"), device="cuda")
    got, kern = _conv_in_once((lat, None, sa, sb, w, b), dtype, 1, gn_part=part)
    assert kern == "rows"
    rows = torch.tensor([0, 1, 255, 256, 510, 511])
    ref, bound = R.conv_in_ref_and_bound(host[0], None, *host[2:], dtype, rows=rows)
    sub = got.view(n, S, S, 128)[:, rows.cuda()].reshape(n, len(rows) * S, 128)
    _note("conv_in_rows", dt, R.check(sub, ref, bound, f"conv_in_rows S 512 {dt}"))
    if part is not None:
        _check_partials(got, part, n, S, dtype, f"front64_rows_512_{dt}")


# ---- sinusoidal embeddings -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", R.SINCOS_DIMS)
def test_timestep_sincos_against_float64(dim):
    E = _eng()
    ref, bound = R.sincos_ref_and_bound(dim, [float(t) for t in R.SINCOS_T])
    for i, t in enumerate(R.SINCOS_T):
        got, _ = _run(lambda o: E.op_timestep_sincos(dim, t, out=o), (dim,), torch.float32)
        _note("timestep_sincos", "f32", R.check(got.cpu(), ref[i], bound[i], f"timestep_sincos dim {dim} t {t}"))
        assert torch.equal(_bits(_run(lambda o: E.op_timestep_sincos(dim, t, out=o), (dim,), torch.float32)[0]), _bits(got))


@pytest.mark.parametrize("dim", R.SINCOS_DIMS)
@pytest.mark.parametrize("name", list(R.SINCOS_VALUES))
def test_sincos_values_against_float64(name, dim):
    _sincos_values(R.SINCOS_VALUES[name], dim, name)


@pytest.mark.parametrize("count", [1, 7])
def test_sincos_values_block_edge(count):
    """dim 256: 128 threads per value, so count 1 is half a 256-thread block and count 7 ends half-way into the fourth"""
    _sincos_values([float(t) for t in R.SINCOS_T][:count], 256, f"count {count}")


def _sincos_values(vals, dim, what):
    E = _eng()
    v = torch.tensor(vals, dtype=torch.float32, device="cuda")
    ref, bound = R.sincos_ref_and_bound(dim, v)
    got, _ = _run(lambda o: E.op_sincos_values(dim, v, out=o), (len(vals), dim), torch.float32)
    _note("sincos_values", "f32", R.check(got.cpu(), ref, bound, f"sincos_values {what} dim {dim}"))
    assert torch.equal(_bits(_run(lambda o: E.op_sincos_values(dim, v, out=o), (len(vals), dim), torch.float32)[0]), _bits(got))


def test_sincos_refuses_nonsense():
    E = _eng()
    _invalid(lambda: E.op_timestep_sincos(255, 5, out=torch.zeros(255, device="cuda")))
    _invalid(lambda: E.op_timestep_sincos(0, 5, out=torch.zeros(0, device="cuda")))


# ---- GEMV ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", R.GEMV_SHAPES)
def test_gemv_against_float64(N, K):
    E = _eng()
    for wname, wdt in DT.items():
        for bdt in (None, torch.float32, torch.bfloat16 if wdt != torch.float16 else torch.float16):
            W, b, x = _cuda(*R.gemv_inputs(N, K, wdt, bdt))
            for act in (0, 1):
                what = f"gemv N {N} K {K} w {wname} bias {bdt} act {act}"
                got, _ = _run(lambda o: E.op_gemv_f32(W, b, x, act, out=o), (N,), torch.float32)
                ref, bound = R.gemv_ref_and_bound(W, b, x, act)
                _note("gemv_w" + wname, "f32", R.check(got, ref, bound, what))
                again, _ = _run(lambda o: E.op_gemv_f32(W, b, x, act, out=o), (N,), torch.float32)
                assert torch.equal(_bits(again), _bits(got)), f"{what}: two runs differ"


# ---- the packs -------------------------------------------------------------------------------------------------------------------
def _pack(kind, shape, sdt, ddt, geglu=0):
    src = R.pack_source(shape, sdt).cuda()
    want = R.pack_ref(kind, src, ddt, geglu)
    got, _ = _run(lambda o: _eng().op_pack(kind, src, ddt, geglu, out=o), tuple(want.shape), ddt)
    assert torch.equal(_bits(got), _bits(want)), f"pack_{kind} {shape} {sdt} -> {ddt} geglu {geglu}"


@pytest.mark.parametrize("dst", list(DT))
@pytest.mark.parametrize("src", list(DT))
def test_pack_linear_and_conv3(src, dst):
    for (N, K), geglu in (((64, 24), 0), ((64, 24), 32), ((640, 40), 16), ((2560, 8), 32)):
        _pack("linear", (N, K), DT[src], DT[dst], geglu)
    for Cout, Cin in ((5, 3), (8, 16)):
        _pack("conv3", (Cout, Cin, 3, 3), DT[src], DT[dst])


@pytest.mark.parametrize("src", list(DT))
def test_pack_conv_in_and_vector(src):
    for Cout, Cin in ((320, 4), (128, 3)):
        _pack("conv_in", (Cout, Cin, 3, 3), DT[src], torch.float32)
    for N, geglu in ((1, 0), (257, 0), (2560, 32), (640, 16)):
        _pack("vector", (N,), DT[src], torch.float32, geglu)


def test_pack_refuses_nonsense():
    E = _eng()
    w = torch.randn(64, 24, device="cuda")
    _invalid(lambda: E.op_pack("linear", w, torch.bfloat16, geglu=8))                     # block rows are 16 or 32
    _invalid(lambda: E.op_pack("linear", w[:48].contiguous(), torch.bfloat16, geglu=32))  # N % (2 geglu) != 0
    _invalid(lambda: E.op_pack("vector", w[:48, 0].contiguous(), torch.float32, geglu=32))
    c = torch.randn(8, 4, 3, 3, device="cuda")
    _invalid(lambda: E.op_pack("conv_in", c, torch.bfloat16))                             # f32 layouts
    _invalid(lambda: E.op_pack("vector", w[:, 0].contiguous(), torch.float16))
    _invalid(lambda: E.op_pack("conv3", c, torch.bfloat16, geglu=16))


# ---- data movement ---------------------------------------------------------------------------------------------------------------
RESIZES = ((4, 4, 7, 7), (7, 7, 13, 13), (13, 13, 25, 25), (2, 3, 3, 5), (1, 1, 3, 3), (8, 8, 3, 3), (5, 5, 5, 5))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dtype,C", [(torch.bfloat16, 8), (torch.float32, 640)], ids=["16B", "2560B"])
def test_resize_nearest_is_torch_nearest(dtype, C, B):
    for Hin, Win, Hout, Wout in RESIZES:
        x = torch.randn(B, Hin, Win, C, device="cuda").to(dtype)
        got, _ = _run(lambda o: _eng().op_resize_nearest(x, Hout, Wout, out=o), (B, Hout, Wout, C), dtype)
        assert torch.equal(got, R.resize_ref(x, Hout, Wout)), (Hin, Win, Hout, Wout, "the integer restatement")
        assert torch.equal(got, R.resize_ref_torch(x, Hout, Wout)), (Hin, Win, Hout, Wout, "F.interpolate")
    _invalid(lambda: _eng().op_resize_nearest(torch.zeros(1, 4, 4, 4, device="cuda", dtype=torch.bfloat16), 7, 7))       # 8-byte rows


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dtype,per", [(torch.bfloat16, 8), (torch.float32, 1028)], ids=["16B", "4112B"])
def test_dup_batch(dtype, per, n):
    x = torch.randn(n, per, device="cuda").to(dtype)
    got, _ = _run(lambda o: _eng().op_dup_batch(x, out=o), (2 * n, per), dtype)
    assert torch.equal(got, R.dup_ref(x))
    _invalid(lambda: _eng().op_dup_batch(torch.zeros(n, 4, device="cuda", dtype=torch.bfloat16)))                       # 8-byte elements


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("n_ctx", [1, 3])
@pytest.mark.parametrize("per", [(77, 768), (5,)], ids=["77x768", "5"])
def test_gather_ctx_clamps(per, n_ctx, dt):
    """a permutation with repeats, plus -1, n_ctx and 2^30: these read the clamped row (0 or n_ctx - 1), never past the table"""
    g = torch.Generator().manual_seed(n_ctx + len(per))
    ctx = torch.randn((n_ctx, 2) + per, generator=g).cuda()
    index = torch.tensor([n_ctx - 1, 0, n_ctx // 2, 0, n_ctx - 1, -1, n_ctx, 2 ** 30], dtype=torch.int32, device="cuda")
    got, _ = _run(lambda o: _eng().op_gather_ctx(ctx, index, DT[dt], out=o), (2 * index.numel(),) + per, DT[dt])
    assert torch.equal(_bits(got), _bits(R.gather_ref(ctx, index, DT[dt])))


# ---- patch embedding -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("case", R.PATCH_CASES, ids=lambda c: "x".join(map(str, c)))
def test_patch_embed_against_float64(case, dt):
    dtype = DT[dt]
    Cin, S, p, D = case
    T = (S // p) ** 2
    for n_img in (1, 3):
        host = R.patch_inputs(Cin, S, p, D, n_img)
        t = _cuda(*host)
        what = f"patch_embed {case} n {n_img} {dt}"
        got, _ = _run(lambda o: _eng().op_patch_embed(*t, p, dtype, out=o), (2 * n_img, T, D), dtype)
        ref, bound = R.patch_ref_and_bound(*host, p, dtype)
        _note("patch_embed", dt, R.check(got, ref, bound, what))
        assert torch.equal(_bits(got[0::2]), _bits(got[1::2])), f"{what}: the CFG halves differ"
        again, _ = _run(lambda o: _eng().op_patch_embed(*t, p, dtype, out=o), (2 * n_img, T, D), dtype)
        assert torch.equal(_bits(again), _bits(got)), f"{what}: two runs differ"
    lat, nz, sa, sb, w, b, pos = t
    _invalid(lambda: _eng().op_patch_embed(lat[:, :, :S - 1, :S - 1].contiguous(), nz[:, :, :S - 1, :S - 1].contiguous(), sa, sb, w, b,
                                           pos[:((S - 1) // p) ** 2].contiguous(), p, dtype))          # S % p != 0


# ---- the VAE's fold and transpose ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("Cm,K", R.FOLD_CASES)
def test_fold_quant_against_float64(Cm, K, dt):
    dtype = DT[dt]
    wq, wco, bco, bq = _cuda(*R.fold_inputs(Cm, K, dtype))
    got, _ = _run(lambda o: _eng().op_fold_quant(wq, wco, out_w=o), (Cm, K), dtype)
    ref, bound = R.fold_ref_and_bound(wq, wco, dtype)
    _note("fold_quant", dt, R.check(got, ref, bound, f"fold_quant {Cm} {K} {dt}"))
    assert torch.equal(_bits(_run(lambda o: _eng().op_fold_quant(wq, wco, out_w=o), (Cm, K), dtype)[0]), _bits(got)), "two runs differ"


@pytest.mark.parametrize("Cm", [8, 65, 1024])
def test_fold_quant_bias_covers_cm(Cm):
    """the bias launch is one workgroup sized from Cm (it was 64 threads whatever Cm: rows from 64 on were left unwritten); beyond
    one workgroup's 1024 threads the operator refuses"""
    wq, _, bco, bq = _cuda(*R.fold_inputs(Cm, 4, torch.float32))
    got, _ = _run(lambda o: _eng().op_fold_quant(wq, bco=bco, bq=bq, out_b=o), (Cm,), torch.float32)
    ref, bound = R.fold_bias_ref_and_bound(wq, bco, bq)
    _note("fold_quant_bias", "f32", R.check(got, ref, bound, f"fold_quant bias Cm {Cm}"))
    assert torch.equal(_bits(_run(lambda o: _eng().op_fold_quant(wq, bco=bco, bq=bq, out_b=o), (Cm,), torch.float32)[0]), _bits(got))


def test_fold_quant_bias_refuses_more_than_a_workgroup():
    wq, _, bco, bq = _cuda(*R.fold_inputs(1025, 4, torch.float32))
    _invalid(lambda: _eng().op_fold_quant(wq, bco=bco, bq=bq))


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("n,HW,C", [(2, 25, 8), (1, 4096, 8)])
def test_to_nchw_f32(n, HW, C, dt):
    x = torch.randn(n, HW, C, device="cuda").to(DT[dt])
    got, _ = _run(lambda o: _eng().op_to_nchw_f32(x, out=o), (n, C, HW), torch.float32)
    assert torch.equal(got, R.nchw_ref(x))


def test_worst_ratios():
    """(runs last in this file) the worst err / bound per (operator, dtype) of the cases that ran in this session"""
    for (op, dt) in sorted(WORST):
        print(f"worst err/bound {dt:4s} {op:18s} {WORST[(op, dt)]:.4f}")
    assert all(w <= 1.0 for w in WORST.values())
