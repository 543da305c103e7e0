"""The row-resident Linear's forms beyond K = 320 behind a LayerNorm (csrc/rowres.hip: rowlin640_kernel behind op_ln_linear at
C = 640, gn_rowlin_kernel<320 / 640> behind op_gn_linear) and the walk that runs them, bf16 and the fp16 twins.

K = 640, with and without the LayerNorm:
  * bit for bit on the lattice family (tests/_rowlin_forms.py) at M = 161 (one full tile and 33 ragged rows) for N = 64 (the ring
    wraps every pair of column blocks) and N = 1920, at M = 1, and at M = 128 (2 CUs + 2) + 33 for N = 64: the smallest size at which a
    workgroup of the two-per-CU grid takes a second tile; there a second launch returns the same bits;
  * against float64 on randn rows (every fifth row with |mean| >> spread), staged as test_gpu_rowres64.py stages K = 320: the
    identity launch returns the kernel's own 16-bit LayerNorm, held to _norm64.ln_ref_and_bound with the depth of its sums (320 per
    lane + the pair), the dense launch on that operand to _gemm64.Gemm64 -- bounds from the rounding points, nothing fitted.
The GroupNorm form (B = 3, HW = 128 and 256, C = 320 and 640, 32 groups, eps 1e-6, a bias, per-channel offsets >> spread in image 1):
  * bit for bit op_groupnorm followed by the same row-resident Linear + bias with no prologue; two launches identical; image b
    alone (B = 1) equals slice b of the batch of 3;
  * against float64, staged: the identity launch (no bias) returns the normalised rows, held to _norm64.gn_ref_and_bound with the
    n_p of the statistics form the shape takes; the dense launch on that operand to Gemm64 with the bias;
  * HW = 96 is refused;
  * the same two tests at HW = 1024 with B = 2 -- there the statistics are gn_stats_kernel's 16 slabs per image, folded by
    gn_coef_kernel, the form the 64 x 64 and 32 x 32 levels of a 512-px step run (HW = 128 and 256 take the one-pass statistics) -- and
    the bit test at HW = 20736 = 128 x 162 with B = 1 (a 1152-px image's 320-channel level): 64 slabs, which fill the GroupNorm
    scratch to its last byte, so the coefficient table must not live there.
The walk (SD1.5 channel plan, latent side 32: 1024 rows at 320 channels, 256 at 640; 2 pairs; taps down_blocks 2 and up_blocks 0):
default mask against fusion = 0 within the 2e-3 of test_gpu_round2's fusion test, reproducible, one pair alone bit for bit the pair
in the batch of 2, and the profile records of the walk to down_blocks 2.  A walk's maps are squares, so 96 rows cannot occur in one:
at latent side 24 (576, 144 rows: no multiple of 128) the walk must take the unfused GroupNorm and 640-channel chains."""
import pytest
import torch

from diffsim_amd import config as C
from diffsim_amd import synth as S
from tests import _gemm64 as G
from tests import _norm64 as N
from tests import _rowlin_forms as F
from tests import _rowres64 as R

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
K = 640
LIN_M = 161
_CACHE = {}


def _eng():
    from diffsim_amd import engine
    return engine


def big_m():
    return 128 * (2 * torch.cuda.get_device_properties(0).multi_processor_count + 2) + 33


def _lattice(M, dt, N_lin):
    key = (M, dt, N_lin)
    if key not in _CACHE:
        if M <= 4096:
            t = {k: v.cuda() for k, v in F.lattice(M, K, DT[dt], M, "cpu", N_lin).items()}
        else:
            t = F.lattice(M, K, DT[dt], M, "cuda", N_lin)
        _CACHE.clear()
        _CACHE[key] = t
    return _CACHE[key]


# ---- K = 640 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("ln", [True, False])
@pytest.mark.parametrize("M,Nn", [(LIN_M, 64), (LIN_M, 1920), (1, 64), (1, 1920), ("big", 64)])
def test_rowlin640_lattice_bits(M, Nn, ln, dt):
    eng = _eng()
    M = big_m() if M == "big" else M
    t = _lattice(M, dt, 1920 if M <= 4096 else 64)
    g, b = (t["gamma"], t["beta"]) if ln else (None, None)
    w = t["wl"][:Nn].contiguous()
    want = (t["lin_ln"] if ln else t["lin"])[:, :Nn].contiguous()
    got = eng.op_ln_linear(t["x"], g, b, w, 1e-5)
    R.assert_bits(got, want, f"op_ln_linear K=640 M={M} N={Nn} ln={ln} {dt}")
    if M > 4096:
        R.assert_bits(eng.op_ln_linear(t["x"], g, b, w, 1e-5), got, f"op_ln_linear K=640 M={M} N={Nn} ln={ln} {dt}, second launch")


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("M,Nn", [(LIN_M, 64), (LIN_M, 640), (LIN_M, 1920), (1, 64), ("big", 64)])
def test_rowlin640_staged_against_float64(M, Nn, dt):
    eng = _eng()
    dtype = DT[dt]
    M = big_m() if M == "big" else M
    t = {k: v.cuda() for k, v in F.random_ln_inputs(M, K, dtype, M, Nn).items()}
    operand = eng.op_ln_linear(t["x"], t["gamma"], t["beta"], torch.eye(K, device="cuda"), 1e-5)
    ref, bound = N.ln_ref_and_bound(t["x"], t["gamma"], t["beta"], 1e-5, dtype, depth=K // 2 + 1)
    worst_ln = N.check(operand, ref, bound, f"op_ln_linear K=640 identity M={M} {dt}")
    del ref, bound
    rows = None if M <= 4096 else torch.unique(torch.cat([G.row_subset(M, 128), torch.arange(M - 40, M)]))
    worst = []
    for ln in (True, False):
        a = operand if ln else t["x"]
        got = eng.op_ln_linear(t["x"], t["gamma"] if ln else None, t["beta"] if ln else None, t["wl"], 1e-5)
        g = G.Gemm64(a, t["wl"], dtype, rows=rows)
        worst.append(g.check(got if rows is None else got[rows.cuda()], f"op_ln_linear K=640 M={M} N={Nn} ln={ln} {dt}"))
    print(f"worst err/bound {dt} K=640 M={M} N={Nn}: LayerNorm {worst_ln:.3f}, dense with / without {worst[0]:.3f} / {worst[1]:.3f}")


# ---- the GroupNorm form --------------------------------------------------------------------------------------------------------------
GROUPS, GN_EPS, GN_B = 32, 1e-6, 3


def _gn(HW, Cc, dt, B=GN_B):
    return {k: v.cuda() for k, v in F.random_gn_inputs(B, HW, Cc, DT[dt], HW + Cc).items()}


GN_CASES = [(GN_B, 128, 320), (GN_B, 128, 640), (GN_B, 256, 320), (GN_B, 256, 640), (2, 1024, 320), (2, 1024, 640)]


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("B,HW,Cc", GN_CASES + [(1, 20736, 320)])
def test_gn_linear_is_the_unfused_chain_to_the_bit(B, HW, Cc, dt):
    eng = _eng()
    t = _gn(HW, Cc, dt, B)
    assert eng.groupnorm_plan(Cc, 0, B, HW, GROUPS, DT[dt])["form"] == ("onepass" if HW <= 256 else "twopass")
    what = f"op_gn_linear B={B} HW={HW} C={Cc} {dt}"
    fused = eng.op_gn_linear(t["x"], t["gamma"], t["beta"], GROUPS, t["w"], t["bias"], GN_EPS)
    nb = eng.op_groupnorm(t["x"], None, t["gamma"], t["beta"], GROUPS, GN_EPS, 0)
    chain = eng.op_gn_linear(nb, None, None, GROUPS, t["w"], t["bias"], GN_EPS)
    R.assert_bits(fused.view(-1, Cc), chain.view(-1, Cc), what + " against groupnorm + row-resident Linear")
    again = eng.op_gn_linear(t["x"], t["gamma"], t["beta"], GROUPS, t["w"], t["bias"], GN_EPS)
    R.assert_bits(again.view(-1, Cc), fused.view(-1, Cc), what + ", second launch")
    for b in range(B if B > 1 else 0):
        one = eng.op_gn_linear(t["x"][b:b + 1].contiguous(), t["gamma"], t["beta"], GROUPS, t["w"], t["bias"], GN_EPS)
        R.assert_bits(one.view(-1, Cc), fused[b], what + f", image {b} alone")


@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("B,HW,Cc", GN_CASES)
def test_gn_linear_staged_against_float64(B, HW, Cc, dt):
    eng = _eng()
    dtype = DT[dt]
    t = _gn(HW, Cc, dt, B)
    operand = eng.op_gn_linear(t["x"], t["gamma"], t["beta"], GROUPS, torch.eye(Cc, device="cuda"), None, GN_EPS)
    n_p = N.gn_n_p(eng.groupnorm_plan(Cc, 0, B, HW, GROUPS, dtype), HW)
    ref, bound = N.gn_ref_and_bound(t["x"], None, t["gamma"], t["beta"], GROUPS, GN_EPS, False, dtype, n_p)
    w1 = N.check(operand, ref, bound, f"op_gn_linear identity HW={HW} C={Cc} {dt}")
    got = eng.op_gn_linear(t["x"], t["gamma"], t["beta"], GROUPS, t["w"], t["bias"], GN_EPS)
    g = G.Gemm64(operand.view(-1, Cc), t["w"], dtype, bias=t["bias"])
    w2 = g.check(got.view(-1, Cc), f"op_gn_linear HW={HW} C={Cc} {dt}")
    print(f"worst err/bound {dt} B={B} HW={HW} C={Cc}: normalised rows {w1:.3f}, dense {w2:.3f}")


@pytest.mark.parametrize("dt", list(DT))
def test_gn_linear_refuses_rows_that_are_no_whole_tiles(dt):
    from diffsim_amd import _lib
    eng = _eng()
    t = _gn(96, 320, dt)
    with pytest.raises(_lib.DsimError):
        eng.op_gn_linear(t["x"], t["gamma"], t["beta"], GROUPS, t["w"], t["bias"], GN_EPS)


# ---- the walk ------------------------------------------------------------------------------------------------------------------------
TAPS = (("down_blocks", 2), ("up_blocks", 0))


def _ds(cfg, sd, **kw):
    from diffsim_amd.diffsim import DiffSim
    return DiffSim(torch_dtype=torch.bfloat16, device="cuda", unet_config=cfg, state_dict=sd, **kw)


@pytest.fixture(scope="module")
def plan():
    cfg = C.UNetConfig(sample_size=32)
    keys = [k for k in C.unet_param_shapes(cfg) if not k.startswith(("up_blocks.2", "up_blocks.3", "conv_norm_out", "conv_out"))]
    sd = S.make_state_dict(cfg, seed=0, keys=keys)
    lat = [S.make_pair_latents(cfg, i) for i in range(2)]
    zA, zB = torch.cat([p[0] for p in lat]), torch.cat([p[1] for p in lat])
    return dict(cfg=cfg, sd=sd, ctx=S.make_context(cfg), zA=zA, zB=zB, n=S.draw_pair_noise(2334, lat[0][0].shape),
                fused=_ds(cfg, sd), plain=_ds(cfg, sd, fusion=0))


def _score(ds, p, blk, layer, sl=slice(None)):
    return ds.score_latent_pairs(p["zA"][sl], p["zB"][sl], p["n"][2], p["n"][3], p["ctx"], blk, layer, 600, "cosine")


@pytest.mark.parametrize("blk,layer", TAPS)
def test_walk_scores(plan, blk, layer):
    a, b = _score(plan["fused"], plan, blk, layer), _score(plan["plain"], plan, blk, layer)
    assert (a - b).abs().max().item() <= 2e-3, (blk, layer, a, b)
    assert torch.equal(a, _score(plan["fused"], plan, blk, layer))                      # reproducible
    for i in range(2):                                                                  # a pair alone: the bits it has in the batch
        assert torch.equal(_score(plan["fused"], plan, blk, layer, slice(i, i + 1)), a[i:i + 1]), (blk, layer, i)


def _records(ds, p, blk, layer):
    e = ds.engine(blk, layer)
    e.profile(True)
    _score(ds, p, blk, layer, slice(0, 1))
    r = e.profile_records(detail=True)
    e.profile(False)
    return r


def test_walk_records(plan):
    r = _records(plan["fused"], plan, "down_blocks", 2)
    fam = [x[0] for x in r]
    assert fam.count("gn_linear_bf16") == 4 and fam.count("groupnorm_stats_bf16") == 4
    ln = [x[4] for x in r if x[0] == "ln_linear_bf16"]
    assert len(ln) == 8 and sum(s.endswith("K320") for s in ln) == 4 and sum(s.endswith("K640") for s in ln) == 4, ln
    # the 640-channel blocks of down_blocks 1 are full blocks (the tap lies in down_blocks 2): no LayerNorm launch but norm3's, whose
    # feed-forward has no row-resident form at 640 channels -- one per block
    ln640 = [x for x in r if x[0] == "layernorm_bf16" and x[4].endswith("C640")]
    assert len(ln640) == 2, ln640
    rp = [x[0] for x in _records(plan["plain"], plan, "down_blocks", 2)]
    assert "gn_linear_bf16" not in rp and "groupnorm_stats_bf16" not in rp and "ln_linear_bf16" not in rp
    # per 320-channel block: the feed-forward's three launches as one and two LayerNorms less; per 640-channel block: two
    # LayerNorms less; statistics + gn_linear for GroupNorm + proj_in: none less; the tap's q / k / v as one launch
    assert len(rp) - len(fam) == 2 * 4 + 2 * 2 + 2


def test_walk_side_24_takes_the_unfused_chains(plan):
    ds = _ds(C.UNetConfig(sample_size=24), plan["sd"])
    cfg = C.UNetConfig(sample_size=24)
    za, zb = S.make_pair_latents(cfg, 0)
    n = S.draw_pair_noise(2334, za.shape)
    e = ds.engine("down_blocks", 2)
    e.profile(True)
    ds.score_latent_pairs(za, zb, n[2], n[3], plan["ctx"], "down_blocks", 2, 600, "cosine")
    r = e.profile_records(detail=True)
    e.profile(False)
    fam = [x[0] for x in r]
    assert "gn_linear_bf16" not in fam and "groupnorm_stats_bf16" not in fam
    ln = [x[4] for x in r if x[0] == "ln_linear_bf16"]
    assert len(ln) == 4 and all(s.endswith("K320") for s in ln), ln       # the 320-channel LayerNorm forms serve any map, as before


def test_walk_side_144_runs_the_groupnorm_form_on_64_statistic_slabs(plan):
    """a 1152-px image: 20736 = 128 x 162 rows at 320 channels, where the GroupNorm statistics take 64 slabs per image.  The walk to
    down_blocks 0 passes one full transformer there and the tapped one's proj_in: both run the GroupNorm form, and the score agrees with
    the unfused walk's"""
    cfg = C.UNetConfig(sample_size=144)
    za, zb = S.make_pair_latents(cfg, 0)
    n = S.draw_pair_noise(2334, za.shape)
    got = {}
    for name, kw in (("fused", {}), ("plain", dict(fusion=0))):
        ds = _ds(cfg, plan["sd"], **kw)
        e = ds.engine("down_blocks", 0)
        e.profile(True)
        got[name] = ds.score_latent_pairs(za, zb, n[2], n[3], plan["ctx"], "down_blocks", 0, 600, "cosine")
        got[name + "_fam"] = [x[0] for x in e.profile_records()]
        e.profile(False)
    assert got["fused_fam"].count("gn_linear_bf16") == 2 and got["fused_fam"].count("groupnorm_stats_bf16") == 2
    assert "gn_linear_bf16" not in got["plain_fam"]
    assert (got["fused"] - got["plain"]).abs().max().item() <= 2e-3, (got["fused"], got["plain"])
