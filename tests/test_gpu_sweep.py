"""Tap sweeps (dsim_unet_qkv_taps / dsim_dit_qkv_taps, the engines' qkv_taps, sweep.py, the scorers' *_taps methods, cli --taps):
every tap's q, k, v and score row from ONE forward must be bit for bit what a one-tap forward at that tap gives."""
import collections
import ctypes as C_

import pytest
import torch

from diffsim_amd import config as C, synth as S
from diffsim_amd.inputs import stack_rows

pytestmark = pytest.mark.gpu


def _pairs(cfg, n, side=None):
    lat = [S.make_pair_latents(cfg, i) for i in range(n)]
    la, lb = torch.cat([p[0] for p in lat]), torch.cat([p[1] for p in lat])
    nz = S.draw_pair_noise(2334, la[:1].shape)
    return la, lb, nz[2], nz[3]


def _ds(cfg, dtype, dedup=True, keys=None, **kw):
    from diffsim_amd.diffsim import DiffSim
    return DiffSim(torch_dtype=dtype, device="cuda", unet_config=cfg, state_dict=S.make_state_dict(cfg, seed=0, keys=keys),
                   dedup_cfg=dedup, **kw)


def _equal_feats(got, want, what):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, what
        assert torch.equal(g, w), what


def _check_sd15(ds, cfg, taps, n=2):
    la, lb, nA, nB = _pairs(cfg, n)
    ctx = S.make_context(cfg)
    lat, nz = stack_rows([la, lb], [nA, nB], 0, n)
    got = ds.features_taps(lat, nz, ctx, taps, 600)
    for tap, f in zip(taps, got):
        _equal_feats(f, ds.features(lat, nz, ctx, tap[0], tap[1], 600), tap)
    rows = ds.score_latent_pairs_taps(la, lb, nA, nB, ctx, taps, 600, "cosine")
    assert rows.shape == (len(taps), n) and rows.dtype == torch.float32
    for t, tap in enumerate(taps):
        assert torch.equal(rows[t], ds.score_latent_pairs(la, lb, nA, nB, ctx, tap[0], tap[1], 600, "cosine")), tap
    return rows


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("dedup", [True, False])
def test_tiny_all_taps_bit_identical(dtype, dedup):
    ds = _ds(C.TINY, dtype, dedup)
    _check_sd15(ds, C.TINY, [("down_blocks", l) for l in range(3)] + [("mid_blocks", 0)] + [("up_blocks", l) for l in range(3)])
    # dedup stays available to a sweep that has no tap in the first down block
    _check_sd15(ds, C.TINY, [("up_blocks", 1), ("down_blocks", 1), ("mid_blocks", 0)])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sd15_small_all_taps_bit_identical(dtype):
    """SD1.5's channel plan: the fused 320-channel LayerNorm + projection and feed-forward run between the taps."""
    ds = _ds(C.SD15_SMALL, dtype)
    from diffsim_amd.sweep import all_taps
    _check_sd15(ds, C.SD15_SMALL, all_taps(C.SD15))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sdxl_taps_across_tfm_blocks_bit_identical(dtype):
    from diffsim_amd.diffsim_xl import diffsim_xl
    from diffsim_amd.sweep import all_taps
    cfg = C.SDXL_TINY
    xl = diffsim_xl(dtype, "cuda", unet_config=cfg, state_dict=S.make_state_dict(cfg, seed=0))
    ctx, pooled = S.make_context(cfg), S.make_pooled(cfg)
    la, lb, nA, nB = _pairs(cfg, 2)
    lat, nz = stack_rows([la, lb], [nA, nB], 0, 2)
    taps = [("up_blocks", [0, 1, 2]), ("up_blocks", [0, 1, 0]), ("up_blocks", [0, 1, 1]), ("mid_blocks", [0, 2]),
            ("mid_blocks", [0, 0]), ("down_blocks", [1, 0, 1]), ("down_blocks", [0, 1, 0]), ("up_blocks", [1, 2, 1])]
    for tp in (taps, all_taps(cfg)):
        got = xl.features_taps(lat, nz, ctx, pooled, tp, 600)
        for tap, f in zip(tp, got):
            _equal_feats(f, xl.features(lat, nz, ctx, pooled, tap[0], tap[1], 600), tap)
    rows = xl.score_latent_pairs_taps(la, lb, nA, nB, ctx, pooled, taps, 600, "cosine")
    for t, tap in enumerate(taps):
        assert torch.equal(rows[t], xl.score_latent_pairs(la, lb, nA, nB, ctx, pooled, tap[0], tap[1], 600, "cosine")), tap


def _dit(dtype):
    from diffsim_amd.diffsim_dit import diffsim_DiT
    cfg = C.DIT_TINY
    dd = diffsim_DiT(8 * cfg.input_size, 600, "cuda", dit_config=cfg, state_dict=S.make_state_dict(cfg, seed=0), torch_dtype=dtype)
    g = torch.Generator().manual_seed(5)
    la, lb = (torch.randn(3, 4, cfg.input_size, cfg.input_size, generator=g) for _ in range(2))
    nA, nB = (torch.randn(1, 4, cfg.input_size, cfg.input_size, generator=g) for _ in range(2))
    return dd, la, lb, nA, nB


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dit_all_blocks_bit_identical(dtype):
    from diffsim_amd import _lib
    dd, la, lb, nA, nB = _dit(dtype)
    lat, nz = stack_rows([la, lb], [nA, nB], 0, 3)
    layers = [2, 0, 1]
    got = dd.features_taps(lat, nz, layers, 600)
    tap0 = dd._engine.target_layer
    for l, f in zip(layers, got):
        _equal_feats(f, dd.features(lat, nz, l, 600), l)
    rows = dd.score_latent_pairs_taps(la, lb, nA, nB, "all", 600, "cosine")
    for l in range(C.DIT_TINY.depth):
        assert torch.equal(rows[l], dd.score_latent_pairs(la, lb, nA, nB, l, 600, "cosine")), l
    eng = dd._engine
    eng.set_tap(tap0)
    for bad in ([], [1, 1], [C.DIT_TINY.depth], [-1]):
        with pytest.raises(_lib.DsimError):
            eng.qkv_taps(lat.cuda(), nz.cuda(), 0.5, 0.5, bad)
    assert eng.target_layer == tap0


def test_sd15_full_size_all_taps():
    """64 x 64 latents, bf16: the 4096-token d = 40 taps and the persistent d = 160 tail at the default tap."""
    from diffsim_amd.sweep import all_taps
    ds = _ds(C.SD15, torch.bfloat16)
    la, lb, nA, nB = _pairs(C.SD15, 2)
    ctx = S.make_context(C.SD15)
    rows = ds.score_latent_pairs_taps(la, lb, nA, nB, ctx, "all", 600, "cosine")
    taps = all_taps(C.SD15)
    assert rows.shape == (7, 2)
    for t, (b, l) in enumerate(taps):
        assert torch.equal(rows[t], ds.score_latent_pairs(la, lb, nA, nB, ctx, b, l, 600, "cosine")), (b, l)


def _recs(eng, fn):
    eng.profile(True)
    fn()
    r = [(fam, shape, fl) for fam, fl, _by, _ms, shape in eng.profile_records(detail=True)]
    eng.profile(False)
    return r


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_no_repeated_prefix(dtype):
    """The sweep's launches are the deepest tap's plus, per shallower tap, its q/k/v projection (and its own norm1 where the block
    carries on through the fused LayerNorm + projection); the FLOPs differ by exactly those projections; the arena is no larger."""
    from diffsim_amd.sweep import all_taps
    cfg = C.SD15_SMALL
    ds = _ds(cfg, dtype, dedup=False)
    la, lb, nA, nB = _pairs(cfg, 2)
    ctx = S.make_context(cfg)
    lat, nz = stack_rows([la, lb], [nA, nB], 0, 2)
    taps = all_taps(C.SD15)
    deepest = ("up_blocks", 2)
    ds.features(lat, nz, ctx, *deepest, 600)                   # (timestep, arenas, code objects)
    eng = ds._base
    deep = _recs(eng, lambda: ds.features(lat, nz, ctx, *deepest, 600))
    sweep = _recs(eng, lambda: ds.features_taps(lat, nz, ctx, taps, 600))
    extra, extra_flops = collections.Counter(), 0.0
    for tap in taps:
        if tap == deepest:
            continue
        one = _recs(eng, lambda: ds.features(lat, nz, ctx, *tap, 600))
        i_ln = max(i for i, r in enumerate(one) if r[0].startswith("layernorm_"))
        proj = one[i_ln + 1:]
        assert 1 <= len(proj) <= 3 and all(r[0].startswith("gemm_") for r in proj), proj
        tok, h, d = eng.tap_shape(*tap)
        fused = dtype != torch.float32 and h * d == 320           # the block carries on through ln_linear
        extra.update(proj + ([one[i_ln]] if fused else []))
        extra_flops += sum(r[2] for r in proj)
        assert sum(r[2] for r in proj) == 2.0 * (2 * 4 * tok) * (h * d) * 3 * (h * d)       # M = 2 CFG x 4 images x tokens
    cd, cs = collections.Counter(deep), collections.Counter(sweep)
    assert not (cd - cs), cd - cs                                 # nothing of the deepest walk is missing
    assert cs - cd == extra, (cs - cd, extra)                     # and only the captures are added
    fd, fs = sum(r[2] for r in deep), sum(r[2] for r in sweep)
    assert abs((fs - fd) - extra_flops) <= 1e-9 * fd, (fs - fd, extra_flops)
    ws_deep = ds.engine(*deepest).workspace_bytes(4)
    assert 0 < eng.taps_workspace_bytes(4, taps) <= ws_deep


def test_one_tap_calls_are_one_path():
    """A one-tap call, a sweep over that one tap and a one-tap call with a context table of one row are one walk: the same launches
    (family, shape, FLOPs) in the same order, and the same bits."""
    from diffsim_amd.scorer import PromptTable
    cfg = C.TINY
    ds = _ds(cfg, torch.bfloat16, dedup=True)
    la, lb, nA, nB = _pairs(cfg, 2)
    ctx = S.make_context(cfg)
    lat, nz = stack_rows([la, lb], [nA, nB], 0, 2)
    table = PromptTable(ds.context(ctx)[None].contiguous(), [0] * lat.shape[0])
    taps = [("down_blocks", l) for l in range(3)] + [("mid_blocks", 0)] + [("up_blocks", l) for l in range(3)]
    ds.features(lat, nz, ctx, *taps[0], 600)                     # (timestep, arenas, code objects)
    eng = ds._base
    for tap in taps:
        calls = {"one": lambda: ds.features(lat, nz, ctx, *tap, 600),
                 "sweep": lambda: ds.features_taps(lat, nz, ctx, [tap], 600)[0],
                 "table": lambda: ds.features(lat, nz, table, *tap, 600)}
        out = {}
        recs = {name: _recs(eng, lambda: out.__setitem__(name, fn())) for name, fn in calls.items()}
        assert recs["one"], tap
        assert recs["sweep"] == recs["one"], tap
        assert recs["table"] == recs["one"], tap
        _equal_feats(out["sweep"], out["one"], tap)
        _equal_feats(out["table"], out["one"], tap)


def test_contract_order_errors_and_handle_state():
    from diffsim_amd import _lib
    cfg = C.TINY
    shapes = C.unet_param_shapes(cfg)
    keys = [k for k in shapes if not k.startswith(("up_blocks.3", "conv_norm_out", "conv_out"))]     # up_blocks[1:][2] is missing
    ds = _ds(cfg, torch.bfloat16, keys=keys)
    la, lb, nA, nB = _pairs(cfg, 3)
    ctx = S.make_context(cfg)
    taps = [("down_blocks", 2), ("up_blocks", 0), ("mid_blocks", 0), ("down_blocks", 0)]
    before = ds.score_latent_pairs(la, lb, nA, nB, ctx, "up_blocks", 1, 600, "mse")
    eng = ds._base
    L = _lib.lib()

    def c_tap():
        n, h, d = C_.c_int(), C_.c_int(), C_.c_int()
        assert L.dsim_unet_tap_shape(eng._h, C_.byref(n), C_.byref(h), C_.byref(d)) == 0
        return n.value, h.value, d.value, eng.target_block, eng.target_layer
    tap0 = c_tap()
    rows = ds.score_latent_pairs_taps(la, lb, nA, nB, ctx, taps, 600, "mse")
    rev = ds.score_latent_pairs_taps(la, lb, nA, nB, ctx, taps[::-1], 600, "mse")
    assert torch.equal(rev, rows.flip(0))
    for bp in (1, 3):                                             # chunking does not change a bit
        assert torch.equal(ds.score_latent_pairs_taps(la, lb, nA, nB, ctx, taps, 600, "mse", batch_pairs=bp), rows)
    assert c_tap() == tap0
    lat, nz = stack_rows([la, lb], [nA, nB], 0, 3)
    lat, nz, ctxd = lat.cuda().contiguous(), nz.cuda().contiguous(), ctx.cuda()
    for bad in ([], [("up_blocks", 0), ("up_blocks", 0)], [("up_blocks", 0), ("up_blocks", 7)], [("side_blocks", 0)],
                [("up_blocks", 2)], [("down_blocks", 1), ("up_blocks", 2)]):
        with pytest.raises(_lib.DsimError):
            eng.qkv_taps(lat, nz, 0.5, 0.5, ctxd, bad)
    assert eng.taps_workspace_bytes(6, [("up_blocks", 2)]) == 0
    assert c_tap() == tap0
    after = ds.score_latent_pairs(la, lb, nA, nB, ctx, "up_blocks", 1, 600, "mse")
    assert torch.equal(before, after)


def _image_files(root, n, seed):
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    paths = []
    for i in range(n):
        base = torch.rand(3, 1, 1, generator=g) * 255
        px = (base + 60 * torch.randn(3, 80, 72, generator=g)).clamp(0, 255).to(torch.uint8)
        p = root / f"img{seed}_{i}.png"
        Image.fromarray(px.permute(1, 2, 0).numpy()).save(p)
        paths.append(str(p))
    return paths


def _files_scorer():
    from diffsim_amd.engine import VAEEncoder
    ctx = S.make_context(C.TINY)
    vae = VAEEncoder(C.VAE_TINY, S.make_state_dict(C.VAE_TINY, seed=3), torch.float32)
    return _ds(C.TINY, torch.bfloat16, vae=vae, encode_prompt=lambda p: ctx)


def test_files_in_pairs_and_triplets(tmp_path):
    from diffsim_amd import harness as H
    from diffsim_amd.sweep import score_path_pairs_taps, score_path_triplets_taps
    ds = _files_scorer()
    im = _image_files(tmp_path, 5, 1)
    pairs = [(im[0], im[1]), (im[2], im[3]), (im[4], im[0])]
    taps = [("up_blocks", 0), ("down_blocks", 1), ("mid_blocks", 0), ("up_blocks", 2)]
    rows = score_path_pairs_taps(ds, pairs, 128, "a cat", taps, 600, "cosine", 2334)
    assert torch.equal(ds.score_pairs_taps(pairs, 128, "a cat", taps, 600, seed=2334), rows)
    for t, (b, l) in enumerate(taps):
        assert torch.equal(rows[t], ds.score_pairs(pairs, 128, "a cat", b, l, 600, seed=2334, similarity="cosine")), (b, l)
    trip = [(im[0], im[1], im[2], "a cat"), (im[3], im[4], im[0], "a dog"), (im[1], im[2], im[3], "a cat")]
    s_ab, s_ac = score_path_triplets_taps(ds, trip, 128, taps, 600, 2334, "mse", unet_triplets=1)
    s_ab3, s_ac3, bad = score_path_triplets_taps(ds, trip, 128, taps, 600, 2334, "mse", unet_triplets=3, return_status=True)
    assert torch.equal(s_ab, s_ab3) and torch.equal(s_ac, s_ac3) and bad == [0] * len(taps)
    for t, (b, l) in enumerate(taps):
        w_ab, w_ac, _ = H.score_path_triplets(ds, trip, 128, b, l, 600, 2334, "mse")
        assert torch.equal(s_ab[t], w_ab) and torch.equal(s_ac[t], w_ac), (b, l)


def _cute_tree(root):
    from PIL import Image
    g = torch.Generator().manual_seed(9)
    for c in range(2):
        for i in range(2):
            for l in range(2):
                d = root / f"cls{c}" / f"inst{i}" / f"light{l}"
                d.mkdir(parents=True)
                for k in range(2):
                    px = (torch.rand(3, 1, 1, generator=g) * 255 + 50 * torch.randn(3, 40, 40, generator=g)).clamp(0, 255)
                    Image.fromarray(px.to(torch.uint8).permute(1, 2, 0).numpy()).save(d / f"im{k}.png")


def test_cli_taps_sections_match_one_tap_runs(tmp_path, monkeypatch, capsys):
    from diffsim_amd import cli
    ds = _files_scorer()
    _cute_tree(tmp_path)
    monkeypatch.setattr(cli, "build_scorer", lambda args: ds)
    base = ["--dataset", "cute", "--image_path", str(tmp_path), "--image_size", "128", "--target_step", "600", "--similarity", "cosine",
            "--seed", "2334"]
    assert cli.run(cli.arg_parse(base + ["--taps", "up_blocks:0", "down_blocks:0", "mid_blocks:0"])) == 0
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "=========seed 2334=========" and sum(ln.startswith("=========seed") for ln in out) == 1
    want = []
    for block in ("up_blocks", "down_blocks", "mid_blocks"):
        assert cli.run(cli.arg_parse(base + ["--target_block", block, "--target_layer", "0"])) == 0
        one = capsys.readouterr().out.splitlines()
        assert one[0] == out[0]
        want += one[1:]
    assert out[1:] == want and len(want) >= 3 * 5
