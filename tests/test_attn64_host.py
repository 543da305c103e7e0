"""The float64 attention reference and bound of tests/_attn64.py, on the CPU: the reference against torch's SDPA and the oracle, an
emulation of every kernel's rounding points within the bound at the production key counts, the perturbations a kernel bug produces
rejected by it; dsim_attention_plan (host code: no device) against a committed table of the kind each case must run, and the table of
reachable instantiations against the attention kernels compiled into the library."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _attn64 as A

PRODUCTION_NK = (77, 784, 1024, 4096)


def _ops(G, Nq, Nk, D, dtype, seed=0, scale=1.3):
    g = torch.Generator().manual_seed(seed + Nk + D)
    q = (torch.randn(G, Nq, D, generator=g) * scale).to(dtype).double()
    k = (torch.randn(G, Nk, D, generator=g) * scale).to(dtype).double()
    v = torch.randn(G, Nk, D, generator=g).to(dtype).double()
    return q, k, v


def test_reference_matches_torch_sdpa_and_the_oracle():
    """sdpa64 (chunked, float64) against one unchunked float64 torch SDPA to 1e-12, and the oracle's attention (oracle/cpu_ref.py
    Attention: its projections set to identities) on a small case"""
    from oracle import cpu_ref as R
    q, k, v = _ops(6, 300, 77, 40, torch.float32)
    ref, _ = A.ref_and_bound(q, k, v, A.Spec("Exact", torch.float32, 40))
    want = F.scaled_dot_product_attention(q, k, v)
    assert float((ref - want).abs().max()) <= 1e-12
    H, D, N, L = 2, 40, 64, 13
    att = R.Attention(H * D, H, H * D).double()
    with torch.no_grad():
        for lin in (att.to_q, att.to_k, att.to_v, att.to_out[0]):
            lin.weight.copy_(torch.eye(H * D))
            if lin.bias is not None:
                lin.bias.zero_()
    x = torch.randn(2, N, H * D, dtype=torch.float64)
    ctx = torch.randn(2, L, H * D, dtype=torch.float64)
    with torch.no_grad():
        want = att(x, ctx)
    got, _ = A.ref_and_bound(A.heads(x, 2, N, H, D), A.heads(ctx, 2, L, H, D), A.heads(ctx, 2, L, H, D), A.Spec("Exact", torch.float32, D))
    got = got.reshape(2, H, N, D).transpose(1, 2).reshape(2, N, H * D)
    assert float((got - want).abs().max()) <= 1e-12


def _emu_cases():
    out = []
    for kind, D in (("Short", 40), ("Short", 64), ("Short", 160), ("ShortK80", 40), ("ShortK80", 80), ("P160", 160), ("Long", 40),
                    ("Q2", 64), ("Q2Fast", 64), ("Fast", 80), ("Fast", 72), ("Exact", 16), ("Exact", 32), ("Exact", 72), ("Exact", 160),
                    ("FP8", 72), ("FP8", 32)):
        dts = (torch.bfloat16,) if kind == "FP8" else (torch.bfloat16, torch.float16)
        nks = {"Short": (64, 96), "ShortK80": (77,), "P160": (256,)}.get(kind, PRODUCTION_NK)
        out += [(kind, D, dt, nk) for dt in dts for nk in nks]
    out += [("Exact", D, torch.float32, nk) for D in (40, 80) for nk in PRODUCTION_NK]
    return out


@pytest.mark.parametrize("kind,D,dtype,Nk", _emu_cases())
def test_emulation_is_within_the_bound(kind, D, dtype, Nk):
    """each kind's rounding points replayed in float32 (_attn64.emulate) on 3 heads x 48 query rows: within the bound, and not
    trivially so (the 16-bit forms reach a tenth of it)"""
    q, k, v = _ops(3, 48, Nk, D, dtype)
    ref, bound = A.ref_and_bound(q, k, v, A.Spec(kind, dtype, D))
    r = A.excess(A.emulate(q, k, v, kind, dtype), ref, bound)
    assert r <= 1.0, r
    if dtype != torch.float32 and kind != "FP8":
        assert r >= 0.1, r


def _rejects(q, k, v, kind, dtype, bad):
    ref, bound = A.ref_and_bound(q, k, v, A.Spec(kind, dtype, q.shape[-1]))
    return A.excess(bad, ref, bound) > 1.0


@pytest.mark.parametrize("dtype,Nk", [(torch.float16, n) for n in PRODUCTION_NK] + [(torch.float32, n) for n in PRODUCTION_NK] +
                         [(torch.bfloat16, 77), (torch.bfloat16, 1024)])
def test_bound_rejects_a_dropped_and_a_doubled_key(dtype, Nk):
    """the last key left out (a mask one key short) or counted twice (a mask admitting key Nk, a tile staged twice): each leaves the
    bound somewhere, on the kind that serves the key count"""
    D = 40
    kind = "ShortK80" if Nk == 77 else ("Long" if Nk == 4096 else ("Fast" if Nk >= 1024 else "Exact"))
    if dtype == torch.float32:
        kind = "Exact"
    q, k, v = _ops(3, 48, Nk, D, dtype)
    assert not _rejects(q, k, v, kind, dtype, A.emulate(q, k, v, kind, dtype))
    assert _rejects(q, k, v, kind, dtype, A.emulate(q, k[:, :-1], v[:, :-1], kind, dtype))
    assert _rejects(q, k, v, kind, dtype, A.emulate(q, torch.cat([k, k[:, -1:]], 1), torch.cat([v, v[:, -1:]], 1), kind, dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind,D,Nk", [("ShortK80", 40, 77), ("Exact", 80, 784), ("Q2Fast", 64, 1024)])
def test_bound_rejects_a_shifted_head_and_the_wrong_kv_element(dtype, kind, D, Nk):
    """a head read one column off (q, k and v of columns h D + 1 ..), and K / V of the wrong batch element"""
    if dtype == torch.float32:
        kind = "Exact"
    g = torch.Generator().manual_seed(D)
    rows = lambda n: (torch.randn(2, n, 2 * D + 8, generator=g) * 1.3).to(dtype).double()     # noqa: E731
    qr, kr, vr = rows(48), rows(Nk), rows(Nk)
    q, k, v = qr[:, :, :D], kr[:, :, :D], vr[:, :, :D]
    assert not _rejects(q, k, v, kind, dtype, A.emulate(q, k, v, kind, dtype))
    sh = A.emulate(qr[:, :, 1:D + 1], kr[:, :, 1:D + 1], vr[:, :, 1:D + 1], kind, dtype)
    assert _rejects(q, k, v, kind, dtype, sh)
    assert _rejects(q, k, v, kind, dtype, A.emulate(q, k.flip(0), v.flip(0), kind, dtype))


def test_softmax_rows_bound_takes_the_rounded_softmax_and_rejects_a_dropped_column():
    x = (torch.randn(64, 784, generator=torch.Generator().manual_seed(3)) * 30).to(torch.bfloat16).double()
    ref, bound = A.softmax_rows_bound(x, 1 / math.sqrt(512), torch.bfloat16)
    assert A.excess(ref.to(torch.bfloat16), ref, bound) <= 1.0
    xd = x.clone()
    xd[:, -1] = -math.inf
    assert A.excess(torch.softmax(xd / math.sqrt(512), -1).to(torch.bfloat16), ref, bound) > 1.0


# the kind dsim_attention_plan names for every case of tests/test_gpu_attn64.py, with that case's strides and offsets
EXPECTED = {
    'sd15_self_4096': {'f32': 'Exact', 'bf16': 'Long', 'f16': 'Long'},
    'sd15_self_1024': {'f32': 'Exact', 'bf16': 'Fast', 'f16': 'Fast'},
    'sd15_self_256': {'f32': 'Exact', 'bf16': 'P160', 'f16': 'P160'},
    'sd15_mid_64': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'sd15_cross_4096': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'sd15_cross_4096_mixed': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'sd15_cross_1024': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'sd15_cross_1024_mixed': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'sd15_cross_256': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'sd15_cross_256_mixed': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'sd15_cross_64': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'sd15_cross_64_mixed': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'sd15s28_self_784': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'sd15s28_self_196': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'sd15s28_self_49': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'sd15s28_mid_16': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'sd15s28_cross_784': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'sd15s28_cross_196': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'sd15s28_cross_49': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'sdxl_self_4096': {'f32': 'Exact', 'bf16': 'Q2Fast', 'f16': 'Q2Fast'},
    'sdxl_self_1024': {'f32': 'Exact', 'bf16': 'Q2Fast', 'f16': 'Q2Fast'},
    'sdxl_cross_4096': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'sdxl_cross_1024': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'sdxl_s26_self_169': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'sdxl_s26_self_49': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'sdxl_q2_exact': {'f32': 'Exact', 'bf16': 'Q2', 'f16': 'Q2'},
    'dit_xl2': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact', 'fp8': 'FP8'},
    'tiny_self_d16': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'tiny_cross_d16': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'tiny_self_d32': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'tiny_cross_d32': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'tiny_self_d64': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'tiny_cross_d64': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'sdxl_tiny_self': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'sdxl_tiny_cross': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'dit_tiny': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact', 'fp8': 'FP8'},
    'sd15_small_self_64': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'sd15_small_cross_64': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'sd15_small_self_16': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'sd15_small_self_4': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'sd15_small_self_1': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'sd15_small_cross_1': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'edge_nk1': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'edge_nk63': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'edge_nk64': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'edge_nk65': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'edge_nk79': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'edge_nk80': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'edge_nk81': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'edge_nk95': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'edge_nk96': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'edge_nk97': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'edge_nk1023': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'edge_nk1024': {'f32': 'Exact', 'bf16': 'Fast', 'f16': 'Fast'},
    'edge_nk2047': {'f32': 'Exact', 'bf16': 'Fast', 'f16': 'Fast'},
    'edge_nk2048': {'f32': 'Exact', 'bf16': 'Long', 'f16': 'Long'},
    'edge_nk2112': {'f32': 'Exact', 'bf16': 'Long', 'f16': 'Long'},
    'edge_nk2125': {'f32': 'Exact', 'bf16': 'Fast', 'f16': 'Fast'},
    'edge_nk81_d80': {'f32': 'Exact', 'bf16': 'Short', 'f16': 'Short'},
    'edge_nk1024_d160': {'f32': 'Exact', 'bf16': 'Fast', 'f16': 'Fast'},
    'edge_nk300_d160': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'edge_nk1024_d16': {'f32': 'Exact', 'bf16': 'Fast', 'f16': 'Fast'},
    'edge_nk1100_d32': {'f32': 'Exact', 'bf16': 'Fast', 'f16': 'Fast'},
    'edge_nk1024_d72': {'f32': 'Exact', 'bf16': 'Fast', 'f16': 'Fast'},
    'edge_nq1': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'edge_nq127': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'edge_nq128': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'edge_nq129': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'edge_nq255': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'edge_nq256': {'f32': 'Exact', 'bf16': 'Q2', 'f16': 'Q2'},
    'edge_nq255_fast': {'f32': 'Exact', 'bf16': 'Fast', 'f16': 'Fast'},
    'edge_h1': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'edge_grid9': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'edge_b5_bkv2': {'f32': 'Exact', 'bf16': 'ShortK80', 'f16': 'ShortK80'},
    'edge_b5_bkv2_tiled': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'rescale_d40': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'rescale_q2': {'f32': 'Exact', 'bf16': 'Q2', 'f16': 'Q2'},
    'rescale_d80': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'rescale_fp8': {'fp8': 'FP8'},
    'fallback_below_long': {'f32': 'Exact', 'bf16': 'Long', 'f16': 'Long'},
    'fallback_above_long': {'f32': 'Exact', 'bf16': 'Long', 'f16': 'Long'},
    'fallback_below_fast': {'f32': 'Exact', 'bf16': 'Fast', 'f16': 'Fast'},
    'fallback_above_fast': {'f32': 'Exact', 'bf16': 'Fast', 'f16': 'Fast'},
    'fallback_above_q2': {'f32': 'Exact', 'bf16': 'Q2Fast', 'f16': 'Q2Fast'},
    'late_spike_long': {'f32': 'Exact', 'bf16': 'Long', 'f16': 'Long'},
    'peaked_d40': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
    'peaked_d72': {'f32': 'Exact', 'bf16': 'Exact', 'f16': 'Exact'},
}


def _layout(c, dt):
    """(ldq, ldk, ldo, q, k, v, out) of a case's layout (tests/test_gpu_attn64._buffers), from fake 16 MB-aligned base addresses"""
    es = 4 if dt == "f32" else 2
    C, base = c["H"] * c["D"], 1 << 24
    if c["layout"] == "qkv":
        return 3 * C, 3 * C, C, base, base + C * es, base + 2 * C * es, 2 * base
    if c["layout"] == "kv":
        return C, 2 * C, C, base, 2 * base, 2 * base + C * es, 3 * base
    return C + 24, C + 40, C + 16, base + 8 * es, 2 * base + 16 * es, 3 * base + 16 * es, 4 * base + 8 * es


def test_plan_table():
    """dsim_attention_plan over the GPU case list (production shapes at their strides, the threshold edges) equals EXPECTED"""
    from diffsim_amd import engine
    from tests.test_gpu_attn64 import CASES, DT
    got = {}
    for c in CASES:
        got[c["name"]] = {}
        for dt in c["dts"]:
            ldq, ldk, ldo, q, k, v, out = _layout(c, dt)
            got[c["name"]][dt] = engine.attention_plan(c["B"], c["Bkv"], c["H"], c["Nq"], c["Nk"], c["D"],
                                                       torch.bfloat16 if dt == "fp8" else DT[dt], ldq=ldq, ldk=ldk, ldo=ldo, q=q,
                                                       k=k, v=v, out=out, fp8=dt == "fp8")
    assert got == EXPECTED


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_plan_p160_needs_aligned_pointers_and_32_bit_offsets(dtype):
    """sdpa160_kernel addresses a (batch element, head) view with 32-bit offsets and 16-byte row segments: an ldo whose view passes
    2^31 bytes, or a pointer off 16 bytes, must send the 256 x 256 d = 160 problem to the tiled kernel (the pointers are never
    dereferenced: the plan only looks at them)"""
    from diffsim_amd import engine
    args = (2, 2, 8, 256, 256, 160, dtype)
    C = 1280
    assert engine.attention_plan(*args, ldq=3 * C, ldk=3 * C, ldo=C) == "P160"
    big = (1 << 31) // (2 * 255)                       # (A_N - 1) ldo 2 + 320 just past 2^31
    big += 8 - big % 8
    assert engine.attention_plan(*args, ldq=3 * C, ldk=3 * C, ldo=big - 8 * 40) == "P160"
    assert engine.attention_plan(*args, ldq=3 * C, ldk=3 * C, ldo=big) == "Exact"
    assert engine.attention_plan(*args, ldq=big, ldk=3 * C, ldo=C) == "Exact"
    assert engine.attention_plan(*args, ldq=3 * C, ldk=big, ldo=C) == "Exact"
    for name in ("q", "k", "v", "out"):
        assert engine.attention_plan(*args, ldq=3 * C, ldk=3 * C, ldo=C, **{name: (1 << 20) + 8}) == "Exact", name


def test_plan_refuses_what_the_launch_refuses():
    from diffsim_amd import _lib, engine
    for kw in (dict(D=24), dict(D=40, ldq=324), dict(D=40, Nk=0), dict(D=40, Nq=0), dict(D=40, Bkv=0)):
        a = dict(B=2, Bkv=2, heads=8, Nq=64, Nk=64, D=40)
        a.update(kw)
        with pytest.raises(_lib.DsimError):
            engine.attention_plan(a["B"], a["Bkv"], a["heads"], a["Nq"], a["Nk"], a["D"], torch.bfloat16, ldq=a.get("ldq"))
    with pytest.raises(_lib.DsimError):
        engine.attention_plan(2, 2, 16, 256, 256, 64, torch.bfloat16, fp8=True)
    with pytest.raises(_lib.DsimError):
        engine.attention_plan(2, 2, 16, 256, 256, 72, torch.float16, fp8=True)


def test_compiled_instantiations_are_the_coverage_tables():
    """Every attention kernel in the built library is in tests/test_gpu_attn64.py's REACHABLE or UNREACHABLE table and every entry
    of those tables is compiled.  (Read from the library's mangled kernel-handle symbols; the 16-bit-only kernels -- short, long,
    q2, sdpa160 -- have no type parameter, so their bf16 / fp16 twins share names.)"""
    import re
    import shutil
    import subprocess
    from diffsim_amd import build
    from tests.test_gpu_attn64 import REACHABLE, UNREACHABLE
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    syms = subprocess.run(["nm", build.build()], capture_output=True, text=True, check=True).stdout
    types = {"f": "f32", "DF16b": "bf16", "DF16_": "f16"}
    got = {dt: set() for dt in REACHABLE}
    for m in re.finditer(r"attn_kernelI(f|DF16b|DF16_)Li(\d+)ELb([01])E", syms):
        got[types[m.group(1)]].add(("Fast" if m.group(3) == "1" else "Exact", int(m.group(2))))
    h16 = set()
    for m in re.finditer(r"attn_short_kernelILi(\d+)ELb([01])E", syms):
        h16.add(("ShortK80" if m.group(2) == "1" else "Short", int(m.group(1))))
    for m in re.finditer(r"attn_long_kernelILi(\d+)ELi0E", syms):
        h16.add(("Long", int(m.group(1))))
    for m in re.finditer(r"attn_q2_kernelILi(\d+)ELb([01])E", syms):
        h16.add(("Q2Fast" if m.group(2) == "1" else "Q2", int(m.group(1))))
    if "sdpa160_kernel" in syms:
        h16.add(("P160", 160))
    for m in re.finditer(r"attn_fp8_kernelILi(\d+)E", syms):
        got["fp8"].add(("FP8", int(m.group(1))))
    assert got["f32"] and got["bf16"] and got["fp8"] and h16, "no kernel symbols parsed"
    got["bf16"] |= h16
    got["f16"] |= h16
    for dt in got:
        want = REACHABLE[dt] | UNREACHABLE[dt]
        assert not REACHABLE[dt] & UNREACHABLE[dt]
        assert got[dt] == want, (dt, "compiled, unlisted", sorted(got[dt] - want), "listed, not compiled", sorted(want - got[dt]))
