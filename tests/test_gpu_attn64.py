"""Every attention kernel against float64, element by element (tests/_attn64.py: the reference and its per-element bound).

The cases are the engines' attention calls at their production shapes, strides and offsets -- SD1.5 at 512 px and at latent side 28,
SDXL, DiT-XL/2, the test configurations the suite runs -- plus the dispatch thresholds of attention_kernel() and constructions that
force its rare branches (the rescale of a growing maximum, the fixed-reference softmax's fp16 fallback).  Each runs through
engine.op_attention_rows (dsim_op_attention_ex: the executors' fused rows) in f32, bf16 and fp16 (and fp8 where the DiT runs it) and
checks
  * the bound on every element of every row, or -- where Nq Nk > 2^22 per head -- on every element of a stated row subset (each
    128-query block's first and last row, the last 64 rows, 64 random rows);
  * that every output is finite and that nothing is written outside the output: the buffer is filled with a sentinel, rows past
    B Nq and columns H D..ldo must keep it;
  * that nothing is read outside the operands: NaN sits in the gap columns of the q / k / v rows (ld > H D) and in the rows past the
    end of K / V (and of Q), so any read of them poisons the output;
  * that repeat launches are bit-identical, and that batch element B - 1 alone gives the same bits where the same kind serves both;
  * that the launch record equals dsim_attention_plan for the same arguments, and names the executors' profile family.
test_launch_coverage then holds the records of the whole case list to the table of reachable (kind, D) per dtype and prints the worst
err / bound per (kind, D, dtype)."""
import math

import pytest
import torch

from tests import _attn64 as A

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENT = -77.0                 # fill of the output buffer: what the kernel must leave alone
ROW_LIMIT = 1 << 22          # Nq Nk per head above which the bound is checked on a row subset

# (kind, D) each dtype reaches through attention_kernel() (fp8: attn_fp8_kernel through the fp8 flag, bf16 in / out)
_H16 = ({("P160", 160), ("Long", 40), ("Q2", 64), ("Q2Fast", 64)} | {(k, d) for k in ("Short", "ShortK80") for d in (40, 64, 80, 160)} |
        {(k, d) for k in ("Fast", "Exact") for d in (16, 32, 40, 64, 72, 80, 160)})
REACHABLE = {"f32": {("Exact", d) for d in (16, 32, 40, 64, 72, 80, 160)}, "bf16": _H16, "f16": set(_H16),
             "fp8": {("FP8", 32), ("FP8", 72)}}
# compiled but never launched: attn_kernel<float, D, true> (the f32 mode keeps the exact running maximum)
UNREACHABLE = {"f32": {("Fast", d) for d in (16, 32, 40, 64, 72, 80, 160)}, "bf16": set(), "f16": set(), "fp8": set()}


def _c(name, B, Bkv, H, Nq, Nk, D, layout="gap", dts=("f32", "bf16", "f16"), ramp=None):
    return dict(name=name, B=B, Bkv=Bkv, H=H, Nq=Nq, Nk=Nk, D=D, layout=layout, dts=dts, ramp=ramp)


# layouts: "qkv" the self-attention's fused [B Nq][3C] rows (k at +C, v at +2C), output [B Nq][C];
#          "kv"  the cross-attention's q [B Nq][C] and k | v rows [Bkv Nk][2C] (v at +C), output [B Nq][C];
#          "gap" q, k, v, out each in rows wider than H D (NaN in the gap columns, the sentinel in the output's)
CASES = [
    # SD1.5 at 512 px: self-attention at every level, the mid block, cross-attention with one K / V per CFG half and per image
    _c("sd15_self_4096", 2, 2, 8, 4096, 4096, 40, "qkv"),
    _c("sd15_self_1024", 2, 2, 8, 1024, 1024, 80, "qkv"),
    _c("sd15_self_256", 2, 2, 8, 256, 256, 160, "qkv"),
    _c("sd15_mid_64", 2, 2, 8, 64, 64, 160, "qkv"),
    _c("sd15_cross_4096", 4, 2, 8, 4096, 77, 40, "kv"),
    _c("sd15_cross_4096_mixed", 4, 4, 8, 4096, 77, 40, "kv"),
    _c("sd15_cross_1024", 8, 2, 8, 1024, 77, 80, "kv"),
    _c("sd15_cross_1024_mixed", 8, 8, 8, 1024, 77, 80, "kv"),
    _c("sd15_cross_256", 16, 2, 8, 256, 77, 160, "kv"),
    _c("sd15_cross_256_mixed", 16, 16, 8, 256, 77, 160, "kv"),
    _c("sd15_cross_64", 32, 2, 8, 64, 77, 160, "kv"),
    _c("sd15_cross_64_mixed", 32, 32, 8, 64, 77, 160, "kv"),
    # SD1.5 at latent side 28 (224 px)
    _c("sd15s28_self_784", 2, 2, 8, 784, 784, 40, "qkv"),
    _c("sd15s28_self_196", 2, 2, 8, 196, 196, 80, "qkv"),
    _c("sd15s28_self_49", 2, 2, 8, 49, 49, 160, "qkv"),
    _c("sd15s28_mid_16", 2, 2, 8, 16, 16, 160, "qkv"),
    _c("sd15s28_cross_784", 4, 4, 8, 784, 77, 40, "kv"),
    _c("sd15s28_cross_196", 4, 2, 8, 196, 77, 80, "kv"),
    _c("sd15s28_cross_49", 4, 2, 8, 49, 77, 160, "kv"),
    # SDXL: d = 64 self-attention on the two-block kernel, 77-key cross-attention, the ragged side 26, Q2 without the fixed reference
    _c("sdxl_self_4096", 2, 2, 10, 4096, 4096, 64, "qkv"),
    _c("sdxl_self_1024", 2, 2, 20, 1024, 1024, 64, "qkv"),
    _c("sdxl_cross_4096", 2, 2, 10, 4096, 77, 64, "kv"),
    _c("sdxl_cross_1024", 4, 4, 20, 1024, 77, 64, "kv"),
    _c("sdxl_s26_self_169", 2, 2, 10, 169, 169, 64, "qkv"),
    _c("sdxl_s26_self_49", 2, 2, 20, 49, 49, 64, "qkv"),
    _c("sdxl_q2_exact", 2, 2, 4, 500, 500, 64, "qkv"),
    # DiT-XL/2 (q | k | v rows of 3 x 1152), bf16 and the fp8 kernel
    _c("dit_xl2", 2, 2, 16, 256, 256, 72, "qkv", ("f32", "bf16", "f16", "fp8")),
    # the suite's test configurations: TINY, SDXL_TINY, DIT_TINY, SD15_SMALL
    _c("tiny_self_d16", 2, 2, 4, 256, 256, 16, "qkv"),
    _c("tiny_cross_d16", 2, 2, 4, 256, 13, 16, "kv"),
    _c("tiny_self_d32", 2, 2, 4, 64, 64, 32, "qkv"),
    _c("tiny_cross_d32", 2, 2, 4, 64, 13, 32, "kv"),
    _c("tiny_self_d64", 2, 2, 4, 16, 16, 64, "qkv"),
    _c("tiny_cross_d64", 2, 2, 4, 16, 13, 64, "kv"),
    _c("sdxl_tiny_self", 2, 2, 2, 64, 64, 64, "qkv"),
    _c("sdxl_tiny_cross", 2, 2, 4, 16, 13, 64, "kv"),
    _c("dit_tiny", 2, 2, 4, 64, 64, 32, "qkv", ("f32", "bf16", "f16", "fp8")),
    _c("sd15_small_self_64", 2, 2, 8, 64, 64, 40, "qkv"),
    _c("sd15_small_cross_64", 2, 2, 8, 64, 77, 40, "kv"),
    _c("sd15_small_self_16", 2, 2, 8, 16, 16, 80, "qkv"),
    _c("sd15_small_self_4", 2, 2, 8, 4, 4, 160, "qkv"),
    _c("sd15_small_self_1", 2, 2, 8, 1, 1, 160, "qkv"),
    _c("sd15_small_cross_1", 2, 2, 8, 1, 77, 160, "kv"),
    # threshold edges: key counts around the 64 / 80 / 96-key limits, ATTN_FAST_MIN, the Long kernel's 2048 and % 64 rules
    *[_c(f"edge_nk{n}", 1, 1, 2, 130, n, 40, "gap") for n in (1, 63, 64, 65, 79, 80, 81, 95, 96, 97, 1023, 1024, 2047, 2048, 2048 + 64,
                                                              2048 + 77)],
    _c("edge_nk81_d80", 2, 2, 2, 100, 81, 80, "gap"),
    _c("edge_nk1024_d160", 1, 1, 2, 200, 1024, 160, "gap"),
    _c("edge_nk300_d160", 1, 1, 2, 100, 300, 160, "gap"),
    _c("edge_nk1024_d16", 1, 1, 2, 130, 1024, 16, "gap"),
    _c("edge_nk1100_d32", 1, 1, 2, 130, 1100, 32, "gap"),
    _c("edge_nk1024_d72", 2, 2, 2, 150, 1024, 72, "gap"),
    # query counts around the Q2 kernel's 256 and the 128-query blocks
    *[_c(f"edge_nq{n}", 1, 1, 2, n, 200, 64, "gap") for n in (1, 127, 128, 129, 255, 256)],
    _c("edge_nq255_fast", 1, 1, 2, 255, 1024, 64, "gap"),
    _c("edge_h1", 2, 2, 1, 300, 300, 72, "gap"),
    _c("edge_grid9", 1, 1, 3, 300, 150, 32, "gap"),                      # 9 workgroups: not a multiple of the 8 XCDs
    _c("edge_b5_bkv2", 5, 2, 3, 200, 77, 80, "kv"),                      # B not a multiple of Bkv (Short walks uneven batch groups)
    _c("edge_b5_bkv2_tiled", 5, 2, 3, 130, 150, 40, "gap"),
    # forced rare branches: every 64-key tile raises every row's maximum (the rescale path); a late ramp that ends just below and
    # just above fp16's range under the fixed-reference softmax (the fallback), the late spike of the existing test
    _c("rescale_d40", 2, 2, 2, 256, 512, 40, "gap", ramp=("tiles", 1.0)),
    _c("rescale_q2", 2, 2, 2, 256, 512, 64, "gap", ramp=("tiles", 1.0)),
    _c("rescale_d80", 2, 2, 2, 200, 300, 80, "gap", ramp=("tiles", 1.0)),
    _c("rescale_fp8", 2, 2, 2, 200, 300, 72, "gap", ("fp8",), ramp=("tiles", 1.0)),
    _c("fallback_below_long", 1, 1, 2, 256, 2048, 40, "gap", ramp=("late", 13.5)),
    _c("fallback_above_long", 1, 1, 2, 256, 2048, 40, "gap", ramp=("late", 16.5)),
    _c("fallback_below_fast", 1, 1, 2, 200, 1100, 80, "gap", ramp=("late", 13.5)),
    _c("fallback_above_fast", 1, 1, 2, 200, 1100, 80, "gap", ramp=("late", 16.5)),
    _c("fallback_above_q2", 1, 1, 2, 256, 1024, 64, "gap", ramp=("late", 16.5)),
    _c("late_spike_long", 2, 1, 2, 300, 2112, 40, "gap", ramp=("spike", 14.0)),
    # near one-hot rows (logits of standard deviation ~12 log2 units): a running maximum of magnitude ~50, re-based in many tiles,
    # whose h16 rounding the KONE kinds (D = 8 mod 16) carry in Q's spare column
    _c("peaked_d40", 2, 2, 2, 192, 333, 40, "gap", ramp=("peaked", 3.0)),
    _c("peaked_d72", 2, 2, 2, 192, 333, 72, "gap", ramp=("peaked", 3.0)),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def runs():
    return [(c["name"], dt) for c in CASES for dt in c["dts"]]


def _ramp(c, q, k, D):
    """write the case's logit construction into q [B][Nq][H][D] and k [Bkv][Nk][H][D] (float32, before rounding)"""
    kind, amp = c["ramp"]
    cq = A.scale_log2(D)
    q[..., 0] = 4.0                                    # every query reads column 0 of the keys with weight 4 c (log2 units per unit)
    Nk = k.shape[1]
    if kind == "tiles":                                # key j: + amp (j // 64) log2 units: each tile's maximum above the last one's
        k[..., 0] += (torch.arange(Nk) // A.KT).float().view(1, Nk, 1) * amp / (4.0 * cq)
    else:                                              # the last 8 keys climb to + amp log2 units ("spike": the last key alone)
        n = 1 if kind == "spike" else 8
        k[:, Nk - n:, :, 0] = (torch.arange(1, n + 1).float() / n * amp / (4.0 * cq)).view(1, n, 1)


def operands(c, seed=0):
    """float32 q [B][Nq][H][D], k, v [Bkv][Nk][H][D] of case c"""
    B, Bkv, H, Nq, Nk, D = (c[x] for x in ("B", "Bkv", "H", "Nq", "Nk", "D"))
    g = torch.Generator().manual_seed(1000 + seed + Nq * 7 + Nk * 3 + D)
    if c["ramp"] is None or c["ramp"][0] == "peaked":
        sc = 1.3 if c["ramp"] is None else c["ramp"][1]
        q = torch.randn(B, Nq, H, D, generator=g) * sc
        k = torch.randn(Bkv, Nk, H, D, generator=g) * sc
    else:
        q = torch.randn(B, Nq, H, D, generator=g) * 0.3
        k = torch.randn(Bkv, Nk, H, D, generator=g) * 0.3
        _ramp(c, q, k, D)
    v = torch.randn(Bkv, Nk, H, D, generator=g)
    return q, k, v


def _buffers(c, q, k, v, tdt):
    """the device buffers of case c's layout, NaN in every gap column and pad row; returns (args for op_attention_rows, out, ldo)"""
    B, Bkv, H, Nq, Nk, D = (c[x] for x in ("B", "Bkv", "H", "Nq", "Nk", "D"))
    C = H * D
    nan = float("nan")
    pad = 3                                             # rows past the end of every operand buffer
    if c["layout"] == "qkv":
        assert B == Bkv and Nq == Nk
        buf = torch.full((B * Nq + pad, 3 * C), nan)
        buf[:B * Nq, :C] = q.reshape(B * Nq, C)
        buf[:B * Nq, C:2 * C] = k.reshape(B * Nq, C)
        buf[:B * Nq, 2 * C:] = v.reshape(B * Nq, C)
        buf = buf.to(tdt).cuda()
        args = (buf, 0, 3 * C, buf, C, buf, 2 * C, 3 * C)
        ldo = C
    elif c["layout"] == "kv":
        qb = torch.full((B * Nq + pad, C), nan)
        qb[:B * Nq] = q.reshape(B * Nq, C)
        kv = torch.full((Bkv * Nk + pad, 2 * C), nan)
        kv[:Bkv * Nk, :C] = k.reshape(Bkv * Nk, C)
        kv[:Bkv * Nk, C:] = v.reshape(Bkv * Nk, C)
        qb, kv = qb.to(tdt).cuda(), kv.to(tdt).cuda()
        args = (qb, 0, C, kv, 0, kv, C, 2 * C)
        ldo = C
    else:
        ldq, ldk = C + 24, C + 40
        qb = torch.full((B * Nq + pad, ldq), nan)
        qb[:B * Nq, 8:8 + C] = q.reshape(B * Nq, C)
        kb = torch.full((Bkv * Nk + pad, ldk), nan)
        vb = torch.full((Bkv * Nk + pad, ldk), nan)
        kb[:Bkv * Nk, 16:16 + C] = k.reshape(Bkv * Nk, C)
        vb[:Bkv * Nk, 16:16 + C] = v.reshape(Bkv * Nk, C)
        qb, kb, vb = qb.to(tdt).cuda(), kb.to(tdt).cuda(), vb.to(tdt).cuda()
        args = (qb, 8, ldq, kb, 16, vb, 16, ldk)
        ldo = C + 16
    out = torch.full((B * Nq + pad, ldo), SENT, dtype=tdt, device="cuda")
    return args, out, ldo


def launch(c, dt, q, k, v):
    """(output [B][Nq][H][D] float64 on the device, launch record, the whole output buffer, ldo, op_attention_rows arguments)"""
    from diffsim_amd import engine
    tdt = torch.bfloat16 if dt == "fp8" else DT[dt]
    args, out, ldo = _buffers(c, q, k, v, tdt)
    o_off = 8 if c["layout"] == "gap" else 0
    kw = dict(B=c["B"], Bkv=c["Bkv"], heads=c["H"], Nq=c["Nq"], Nk=c["Nk"], D=c["D"], fp8=dt == "fp8")
    rec = engine.op_attention_rows(*args, out.view(-1), o_off, ldo, **kw)
    B, H, Nq, D = c["B"], c["H"], c["Nq"], c["D"]
    got = out[:B * Nq, o_off:o_off + H * D].double().reshape(B, Nq, H, D)
    return got, rec, out, ldo, (args, o_off, kw)


def rows_checked(Nq, Nk, seed=0):
    """every row, or -- above ROW_LIMIT per head -- each 128-query block's first and last row, the last 64 rows, 64 random rows"""
    if Nq * Nk <= ROW_LIMIT:
        return torch.arange(Nq)
    g = torch.Generator().manual_seed(seed)
    r = torch.cat([torch.arange(0, Nq, 128), torch.arange(127, Nq, 128), torch.arange(Nq - 64, Nq), torch.randint(0, Nq, (64,), generator=g)])
    return torch.unique(r)


RECORDS = {}                 # (case, dtype) -> launch record
WORST = {}                   # (case, dtype) -> largest err / bound


def check_case(name, dt):
    from diffsim_amd import engine
    c = BY_NAME[name]
    B, Bkv, H, Nq, Nk, D = (c[x] for x in ("B", "Bkv", "H", "Nq", "Nk", "D"))
    tdt = torch.bfloat16 if dt == "fp8" else DT[dt]
    q, k, v = operands(c)
    q, k, v = (t.to(tdt).float() for t in (q, k, v))
    got, rec, out, ldo, (args, o_off, kw) = launch(c, dt, q, k, v)
    RECORDS[(name, dt)] = rec
    # the record is the kernel the dispatch rule names for the same pointers and strides, under the executors' family name
    es = out.element_size()
    ptr = lambda t, off: t.data_ptr() + off * es                                          # noqa: E731
    plan = engine.attention_plan(B, Bkv, H, Nq, Nk, D, tdt, ldq=args[2], ldk=args[7], ldo=ldo, q=ptr(args[0], args[1]),
                                 k=ptr(args[3], args[4]), v=ptr(args[5], args[6]), out=ptr(out, o_off), fp8=dt == "fp8")
    assert rec["kind"] == plan and rec["D"] == D, (name, dt, rec, plan)
    fam = f"attention_fp8_d{D}" if dt == "fp8" else f"attention_{dt}_d{D}" + {"P160": "_p160", "Short": "_short", "ShortK80": "_short",
                                                                              "Long": "_long", "Q2": "_q2", "Q2Fast": "_q2fast",
                                                                              "Fast": "_fast"}.get(rec["kind"], "")
    assert rec["family"] == fam and rec["k80"] == (rec["kind"] == "ShortK80"), (name, dt, rec)
    assert rec["dtype"] == tdt
    # finite, and nothing written outside the output
    assert torch.isfinite(got).all(), (name, dt, "non-finite output (an over-read of a NaN gap or pad?)")
    assert (out[B * Nq:] == SENT).all(), (name, dt, "rows past B Nq written")
    cols = torch.ones(ldo, dtype=torch.bool)
    cols[o_off:o_off + H * D] = False
    assert (out[:B * Nq, cols.cuda()] == SENT).all(), (name, dt, "columns outside H D written")
    # repeat launches: the same bits
    got2 = launch(c, dt, q, k, v)[0]
    assert torch.equal(got, got2), (name, dt, "repeat launch differs")
    # the bound, per head, on the checked rows
    rows = rows_checked(Nq, Nk).cuda()
    spec = A.Spec(rec["kind"], tdt, D)
    qh = A.heads(q.double().cuda()[:, rows], B, len(rows), H, D)
    kh = A.expand_kv(A.heads(k.double().cuda(), Bkv, Nk, H, D), B, Bkv, H)
    vh = A.expand_kv(A.heads(v.double().cuda(), Bkv, Nk, H, D), B, Bkv, H)
    ref, bound = A.ref_and_bound(qh, kh, vh, spec)
    gh = A.heads(got[:, rows], B, len(rows), H, D)
    err = (gh - ref).abs()
    ratio = err / bound
    WORST[(name, dt)] = float(ratio.max())
    if not (ratio <= 1).all():
        i = int(ratio.argmax())
        gi, ri, di = i // (len(rows) * D), (i // D) % len(rows), i % D
        raise AssertionError(f"{name} {dt} {rec['family']}: err {float(err.flatten()[i]):.3e} > bound {float(bound.flatten()[i]):.3e} "
                             f"(ratio {WORST[(name, dt)]:.2f}) at (b, h) {divmod(gi, H)} row {int(rows[ri])} d {di}; "
                             f"ref {float(ref.flatten()[i]):.4e} got {float(gh.flatten()[i]):.4e}")
    # batch element B - 1 alone, where the same kind serves it: the same bits
    if B > 1:
        c1 = dict(c, B=1, Bkv=1)
        b, bk = B - 1, (B - 1) % Bkv
        if engine.attention_plan(1, 1, H, Nq, Nk, D, tdt, ldq=args[2], ldk=args[7], ldo=ldo, fp8=dt == "fp8") == rec["kind"]:
            g1 = launch(c1, dt, q[b:b + 1], k[bk:bk + 1], v[bk:bk + 1])[0]
            assert torch.equal(g1[0], got[b]), (name, dt, "batch element alone differs")


@pytest.mark.parametrize("name,dt", runs())
def test_attention_case(name, dt):
    check_case(name, dt)


def test_launch_coverage():
    """The launch records of the case list equal the table of reachable (kind, D) per dtype (cases not run in this session are
    launched here); prints the worst err / bound per (kind, D, dtype)."""
    for name, dt in runs():
        if (name, dt) not in RECORDS:
            c = BY_NAME[name]
            tdt = torch.bfloat16 if dt == "fp8" else DT[dt]
            RECORDS[(name, dt)] = launch(c, dt, *(t.to(tdt).float() for t in operands(c)))[1]
    seen = {dt: set() for dt in REACHABLE}
    for (name, dt), r in RECORDS.items():
        seen[dt].add((r["kind"], r["D"]))
    for dt in REACHABLE:
        assert seen[dt] == REACHABLE[dt], (dt, "missing", sorted(REACHABLE[dt] - seen[dt]), "unexpected", sorted(seen[dt] - REACHABLE[dt]))
    worst = {}
    for (name, dt), w in WORST.items():
        r = RECORDS[(name, dt)]
        key = (dt, r["kind"], r["D"])
        if w > worst.get(key, (-1.0, ""))[0]:
            worst[key] = (w, name)
    for key in sorted(worst):
        print(f"worst err/bound {key[0]:4s} {key[1]:8s} d{key[2]:<3d} {worst[key][0]:.3f}  ({worst[key][1]})")


def test_launch_record_and_plan_refusals():
    """dsim_op_attention_ex refuses what dsim_attention_plan refuses (an unsupported head dim, fp8 outside bf16) and writes nothing"""
    from diffsim_amd import _lib, engine
    q = torch.randn(1, 64, 2 * 24).to(torch.bfloat16).cuda()
    out = torch.full((64 * 48,), SENT, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(_lib.DsimError):
        engine.attention_plan(1, 1, 2, 64, 64, 24, torch.bfloat16)
    with pytest.raises(_lib.DsimError):
        engine.op_attention_rows(q.view(-1), 0, 48, q.view(-1), 0, q.view(-1), 0, 48, out, 0, 48, B=1, Bkv=1, heads=2, Nq=64, Nk=64, D=24)
    qf = torch.randn(64, 64).to(torch.float16).cuda()
    of = torch.full((64 * 64,), SENT, dtype=torch.float16, device="cuda")
    with pytest.raises(_lib.DsimError):
        engine.op_attention_rows(qf.view(-1), 0, 64, qf.view(-1), 0, qf.view(-1), 0, 64, of, 0, 64, B=1, Bkv=1, heads=2, Nq=64, Nk=64, D=32,
                                 fp8=True)
    assert (out == SENT).all() and (of == SENT).all()


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("rows,cols", [(512, 4096), (784, 784)])
def test_softmax_rows(dt, rows, cols):
    """softmax_rows_kernel (the VAE mid-block's softmax: 4096 columns at 512 px, 784 at 224 px) against float64, every element,
    under tests/_attn64.softmax_rows_bound"""
    from diffsim_amd import engine
    tdt = DT[dt]
    C = 512
    g = torch.Generator().manual_seed(rows + cols)
    x = (torch.randn(rows, cols, generator=g) * math.sqrt(C) * 1.3).to(tdt)
    got = engine.op_softmax_rows(x.cuda(), 1.0 / math.sqrt(C)).double()
    assert torch.isfinite(got).all()
    ref, bound = A.softmax_rows_bound(x.double().cuda(), 1.0 / math.sqrt(C), tdt)
    ratio = float(((got - ref).abs() / bound).max())
    print(f"softmax_rows {dt} {rows}x{cols}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
