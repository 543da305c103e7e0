"""Text-guided regions end to end on synthetic weights (TINY, SDXL_TINY): the executor's walk behind the tap's cross-attention query
(dsim_unet_qkv_text / UNetEngine.qkv_text) against qkv() to the bit and against the oracle's restatement
(tests/_textattn64.oracle_text_operands), and the scorer paths built on it (textattn.py, harness.score_path_triplets(text=),
--text_attn)."""
import os

import pytest
import torch

from diffsim_amd import config as C
from diffsim_amd import synth as S
from tests import _textattn64 as X

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TINY_TAPS = [("down_blocks", 0), ("down_blocks", 1), ("down_blocks", 2), ("mid_blocks", 0), ("up_blocks", 0), ("up_blocks", 1),
             ("up_blocks", 2)]
XL_TAPS = [("up_blocks", [0, 1, 2]), ("up_blocks", [0, 1, 0])]             # the last transformer block of its model, and the first of three
STEP = 600


@pytest.fixture(scope="module")
def tiny():
    from oracle import cpu_ref as R
    sd = S.make_state_dict(C.TINY, seed=0)
    g = torch.Generator().manual_seed(11)
    lat, nz = torch.randn(4, 4, 16, 16, generator=g), torch.randn(4, 4, 16, 16, generator=g)
    ctxs = [S.make_context(C.TINY), S.make_context(C.TINY, seed=78), S.make_context(C.TINY, seed=79)]
    return dict(sd=sd, R=R, oracle=R.build_unet(R.TINY, sd), ctx=ctxs[0], ctxs=ctxs, lat=lat, nz=nz, scorers={})


def _sd15(tiny, dtype, **kw):
    """one DiffSim per dtype for the module (a fake VAE and tokenizer; a prompt string is one of three synthetic contexts)"""
    from diffsim_amd.diffsim import DiffSim
    from tests._fakes import FakeVAE
    key = (dtype, tuple(sorted(kw.items())))
    if key not in tiny["scorers"]:
        prompts = {"a cat": tiny["ctxs"][0], "the big dog": tiny["ctxs"][1], "a red snowboard": tiny["ctxs"][2]}
        ds = DiffSim(torch_dtype=dtype, device="cuda", unet_config=C.TINY, state_dict=tiny["sd"], vae=FakeVAE(),
                     encode_prompt=lambda p: prompts[p], **kw)
        ds.tokenize = X.WordTokenizer(C.TINY.ctx_len)
        tiny["scorers"][key] = ds
    return tiny["scorers"][key]


# ---- 1. the executor ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "bfloat16", "float16"])
def test_tiny_qkv_text_is_qkv_at_every_tap_and_leaves_no_state(tiny, dtype):
    ds = _sd15(tiny, dtype)
    lat, nz, ctx = tiny["lat"][:3], tiny["nz"][:3], tiny["ctx"]
    for block, layer in TINY_TAPS:
        before = ds.features(lat, nz, ctx, block, layer, STEP)
        q, k, v, xq, xkv = ds.features_text(lat, nz, ctx, block, layer, STEP)
        after = ds.features(lat, nz, ctx, block, layer, STEP)
        for got, b, a in zip((q, k, v), before, after):
            assert torch.equal(got, b) and torch.equal(a, b), (block, layer)
        eng = ds.engine(block, layer)
        assert xq.shape == (3, 2, eng.tokens, eng.heads * eng.head_dim) and xq.dtype == dtype
        assert xkv.shape == (2, C.TINY.ctx_len, 2 * eng.heads * eng.head_dim)
        assert torch.isfinite(xq.float()).all() and torch.isfinite(xkv.float()).all()
        # image i does not depend on its batch neighbours
        one = ds.features_text(lat[1:2], nz[1:2], ctx, block, layer, STEP)
        assert torch.equal(one[3][0], xq[1]) and torch.equal(one[4], xkv), (block, layer)


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "bfloat16", "float16"])
def test_tiny_operands_against_the_oracle(tiny, dtype):
    """fp32 mode: within 2e-4 max|want| of the oracle's restatement, the gate tests/test_gpu_e2e.py puts on q / k / v; the 16-bit
    modes report their error."""
    R, unet, ctx = tiny["R"], tiny["oracle"], tiny["ctx"]
    ds = _sd15(tiny, dtype)
    for block, layer in TINY_TAPS:
        _, _, _, xq, xkv = ds.features_text(tiny["lat"][:2], tiny["nz"][:2], ctx, block, layer, STEP)
        for i in range(2):
            z, n = tiny["lat"][i:i + 1], tiny["nz"][i:i + 1]
            wq, wkv = X.oracle_text_operands(unet, lambda: R.features(unet, z, n, ctx, STEP, block, layer, full=True), block, layer)
            eq = (xq[i].float().cpu() - wq).abs().max().item() / float(wq.abs().max())
            ek = (xkv.float().cpu() - wkv).abs().max().item() / float(wkv.abs().max())
            print(f"{str(dtype)[6:]} {block} {layer} image {i}: xq err {eq:.2e}  xkv err {ek:.2e}  (relative to max|want|)")
            if dtype == torch.float32:
                assert eq <= 2e-4 and ek <= 2e-4, (block, layer, i, eq, ek)


def test_context_table_rows_are_the_one_prompt_calls(tiny):
    for dtype in (torch.float32, torch.bfloat16):
        ds = _sd15(tiny, dtype)
        lat, nz = tiny["lat"], tiny["nz"]
        prompts = [tiny["ctxs"][0], tiny["ctxs"][1], tiny["ctxs"][0], tiny["ctxs"][2]]
        for block, layer in (("up_blocks", 0), ("down_blocks", 1)):
            q, k, v, xq, xkv = ds.features_text(lat, nz, prompts, block, layer, STEP)
            plain = ds.features(lat, nz, prompts, block, layer, STEP)
            assert all(torch.equal(a, b) for a, b in zip((q, k, v), plain))
            assert xkv.shape[0] == 8
            for i, p in enumerate(prompts):
                one = ds.features_text(lat[i:i + 1], nz[i:i + 1], p, block, layer, STEP)
                assert torch.equal(one[3][0], xq[i]) and torch.equal(one[4], xkv[2 * i:2 * i + 2]), (block, layer, i)


def test_workspace_query_and_a_short_workspace(tiny):
    from diffsim_amd import _lib
    ds = _sd15(tiny, torch.bfloat16)
    eng = ds.engine("up_blocks", 0)
    eng.set_sample_size(16)
    need = eng.text_workspace_bytes(3)
    assert need >= eng.workspace_bytes(3) > 0
    assert eng.text_workspace_bytes(0) == 0 and eng.text_workspace_bytes(3, 0) == 0
    assert eng.text_workspace_bytes(3, 2) >= eng.workspace_bytes(3, 2) > 0
    mx = eng.max_images()
    if mx < 4096:
        assert eng.text_workspace_bytes(mx + 1) == 0
    L = _lib.lib()
    n, N, Cc = 3, eng.tokens, eng.heads * eng.head_dim
    lat, nz, ctx = tiny["lat"][:n].cuda(), tiny["nz"][:n].cuda(), tiny["ctx"].cuda().float()
    from diffsim_amd import scheduler as sched
    eng.set_timestep(sched.timestep_from_index(STEP))
    outs = [torch.full((n, 2, N, Cc), -7.0, dtype=torch.bfloat16, device="cuda") for _ in range(4)]
    xkv = torch.full((2, C.TINY.ctx_len, 2 * Cc), -7.0, dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")            # (256-byte aligned: the query's slack is spare)
    assert ws.data_ptr() % 256 == 0
    args = [eng._h, lat.data_ptr(), nz.data_ptr(), 1.0, 0.0, ctx.data_ptr(), 1, None, n] + [t.data_ptr() for t in outs] + [xkv.data_ptr()]
    rc = L.dsim_unet_qkv_text(*args, ws.data_ptr(), need - 257, None)
    torch.cuda.synchronize()
    assert rc == -3 and b"workspace" in L.dsim_strerror(rc).lower()
    assert all((t == -7.0).all() for t in outs) and (xkv == -7.0).all()                                   # nothing was enqueued
    bad = list(args)
    bad[12] = None                                                                                       # no xq
    assert L.dsim_unet_qkv_text(*bad, ws.data_ptr(), need, None) == -1
    bad = list(args)
    bad[13] = None                                                                                       # no xkv
    assert L.dsim_unet_qkv_text(*bad, ws.data_ptr(), need, None) == -1
    torch.cuda.synchronize()
    assert all((t == -7.0).all() for t in outs) and (xkv == -7.0).all()
    assert L.dsim_unet_qkv_text(*args, ws.data_ptr(), need, None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(outs[3].float()).all() and torch.isfinite(xkv.float()).all()


def test_sdxl_tiny_qkv_text(tiny):
    from oracle import cpu_ref as R
    from diffsim_amd.diffsim_xl import diffsim_xl
    from tests._fakes import FakeVAE
    sd = S.make_state_dict(C.SDXL_TINY, seed=0)
    unet = R.build_unet(R.SDXL_TINY, sd)
    ctx, pooled = S.make_context(C.SDXL_TINY), S.make_pooled(C.SDXL_TINY)
    lat, nz = tiny["lat"][:2], tiny["nz"][:2]
    for dtype in DTYPES:
        xl = diffsim_xl(dtype, "cuda", unet_config=C.SDXL_TINY, state_dict=sd, vae=FakeVAE(), encode_prompt=lambda p: (ctx, pooled))
        for block, layer in XL_TAPS:
            before = xl.features(lat, nz, ctx, pooled, block, layer, STEP)
            q, k, v, xq, xkv = xl.features_text(lat, nz, ctx, pooled, block, layer, STEP)
            after = xl.features(lat, nz, ctx, pooled, block, layer, STEP)
            for got, b, a in zip((q, k, v), before, after):
                assert torch.equal(got, b) and torch.equal(a, b), (dtype, layer)
            one = xl.features_text(lat[1:2], nz[1:2], ctx, pooled, block, layer, STEP)
            assert torch.equal(one[3][0], xq[1]) and torch.equal(one[4], xkv)
            for i in range(2):
                z, n = lat[i:i + 1], nz[i:i + 1]
                wq, wkv = X.oracle_text_operands(unet, lambda: R.features_xl(unet, z, n, ctx, pooled, STEP, block, layer, full=True),
                                                 block, layer)
                eq = (xq[i].float().cpu() - wq).abs().max().item() / float(wq.abs().max())
                ek = (xkv.float().cpu() - wkv).abs().max().item() / float(wkv.abs().max())
                print(f"sdxl_tiny {str(dtype)[6:]} {layer} image {i}: xq err {eq:.2e}  xkv err {ek:.2e}")
                if dtype == torch.float32:
                    assert eq <= 2e-4 and ek <= 2e-4, (layer, i, eq, ek)
        if dtype == torch.float32:
            # the scorer path: a (context, pooled) prompt needs the weights themselves; regions; threshold 0 is the whole image
            a, b = _image_files_of(tiny)
            w = torch.zeros(C.SDXL_TINY.ctx_len)
            w[1:4] = 1.0
            from diffsim_amd import textattn as TA
            s, masks, counts = TA.score_latent_pairs_text(xl, lat[:1], lat[1:2], nz[:1], nz[1:2], (ctx, pooled), "up_blocks", [0, 1, 2], STEP,
                                                          "cosine", weights=w, return_regions=True)
            assert torch.isfinite(s).all() and torch.equal(counts, masks.sum(-1).to(torch.int32)) and 0 < int(counts.min())
            whole = TA.score_latent_pairs_text(xl, lat[:1], lat[1:2], nz[:1], nz[1:2], (ctx, pooled), "up_blocks", [0, 1, 2], STEP, "cosine",
                                               weights=w, rel_threshold=0.0)
            assert torch.equal(whole, xl.score_latent_pairs(lat[:1], lat[1:2], nz[:1], nz[1:2], ctx, pooled, "up_blocks", [0, 1, 2], STEP))
            with pytest.raises(ValueError, match="weights"):
                TA.score_latent_pairs_text(xl, lat[:1], lat[1:2], nz[:1], nz[1:2], (ctx, pooled), "up_blocks", [0, 1, 2], STEP)
            xl.tokenize = X.WordTokenizer(C.SDXL_TINY.ctx_len)
            m = xl.text_attention_map(a, b, 128, "a cat", "up_blocks", [0, 1, 2], STEP, 2334)
            assert m.shape[0] == 2 and m.shape[3] == C.SDXL_TINY.ctx_len and ((m.sum(-1) - 1).abs() < 1e-5).all()
            r = xl.text_region_score(a, b, 128, "a cat", "up_blocks", [0, 1, 2], STEP, 2334, "cosine", words=["cat"])
            assert r.shape == (1,) and torch.isfinite(r).all()


def _image_files_of(tiny):
    import glob
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    imgs = sorted(glob.glob(os.path.join(root, "g1_img_*.png")))
    return imgs[0], imgs[1]


# ---- 2. the scorer paths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
def test_text_scores_are_the_region_scores_over_the_text_masks(tiny, dtype):
    from diffsim_amd import engine as E, regions as RG, textattn as TA
    from diffsim_amd.scorer import stack_rows
    ds = _sd15(tiny, dtype)
    latA, latB = tiny["lat"][:3], tiny["lat"][[1, 2, 3]]
    nA, nB = tiny["nz"][:1], tiny["nz"][1:2]
    block, layer = "up_blocks", 0
    tap = ds.tap_of(block, layer)
    heads = ds.engine_at(tap).heads
    for sim in ("cosine", "mse"):
        got, masks, counts = TA.score_latent_pairs_text(ds, latA, latB, nA, nB, "a cat", block, layer, STEP, sim, words=["cat"],
                                                        batch_pairs=3, return_regions=True)
        # the same features, the text attention call, the region tail
        q, k, v, xq, xkv = ds.tap_features_text(*stack_rows([latA.cuda(), latB.cuda()], [nA.cuda(), nB.cuda()], 0, 3),
                                                ds.bind_prompt("a cat", 3, "pairs"), tap, STEP)
        w = TA.prompt_token_weights(ds.tokenize, "a cat", ["cat"]).cuda()
        out = E.text_attention(xq, xkv, heads, w, 1.0, want=("mask", "counts", "status"))
        assert out["status"].tolist() == [0] * 6
        ia = torch.arange(0, 6, 2, dtype=torch.int32).cuda()
        assert torch.equal(got, E.pair_score_regions(q, k, v, out["mask"], ia, ia + 1, heads, sim)), sim
        assert torch.equal(masks.reshape(6, -1), out["mask"]) and torch.equal(counts.reshape(-1), out["counts"])
        N = masks.shape[-1]
        assert 0 < int(counts.min()) and int(counts.max()) < N                                    # regions, not whole images
        # ... which is also regions.py's call with those masks handed in
        assert torch.equal(got, RG.score_latent_pair_regions(ds, latA, latB, nA, nB, masks[:, 0], masks[:, 1], "a cat", block, layer,
                                                             STEP, sim, batch_pairs=3))
        # batch_pairs 1 vs 3
        one = TA.score_latent_pairs_text(ds, latA, latB, nA, nB, "a cat", block, layer, STEP, sim, words=["cat"], batch_pairs=1)
        assert torch.equal(one, got)
        # threshold 0: every token on: the region score with full masks, which is the pair score
        full = torch.ones(3, N, dtype=torch.bool)
        zero = TA.score_latent_pairs_text(ds, latA, latB, nA, nB, "a cat", block, layer, STEP, sim, rel_threshold=0.0)
        assert torch.equal(zero, RG.score_latent_pair_regions(ds, latA, latB, nA, nB, full, full, "a cat", block, layer, STEP, sim))
    # a prompt per pair: weights per pair, each pair bit for bit its own one-prompt call
    prompts = ["a cat", "the big dog", "a red snowboard"]
    mixed = TA.score_latent_pairs_text(ds, latA, latB, nA, nB, prompts, block, layer, STEP, "cosine", batch_pairs=3)
    for i, p in enumerate(prompts):
        alone = TA.score_latent_pairs_text(ds, latA[i:i + 1], latB[i:i + 1], nA, nB, p, block, layer, STEP, "cosine")
        assert torch.equal(alone[0], mixed[i]), i
    # a context tensor as the prompt needs the weights themselves
    with pytest.raises(ValueError, match="weights"):
        TA.score_latent_pairs_text(ds, latA, latB, nA, nB, tiny["ctx"], block, layer, STEP)
    w = TA.prompt_token_weights(ds.tokenize, "a cat")
    given = TA.score_latent_pairs_text(ds, latA, latB, nA, nB, tiny["ctx"], block, layer, STEP, "cosine", weights=w)
    assert torch.equal(given, TA.score_latent_pairs_text(ds, latA, latB, nA, nB, "a cat", block, layer, STEP, "cosine"))
    # the maps
    m = TA.text_attention_maps(ds, latA, nA, "a cat", block, layer, STEP)
    g = RG.tap_grid(ds, tap, 16)
    assert m.shape == (3, g[0], g[1], C.TINY.ctx_len) and ((m.sum(-1) - 1).abs() < 1e-5).all()


def test_dit_raises():
    from diffsim_amd import textattn as TA
    from diffsim_amd.diffsim_dit import diffsim_DiT
    from tests._fakes import FakeVAE
    dd = diffsim_DiT(128, 600, "cuda", dit_config=C.DIT_TINY, state_dict=S.make_state_dict(C.DIT_TINY, seed=0), vae=FakeVAE(),
                     torch_dtype=torch.float32)
    z = torch.zeros(1, 4, 16, 16)
    with pytest.raises(NotImplementedError, match="text"):
        dd.text_region_score("a.png", "b.png", 128, None, "none", [2], 600, 2334, "cosine")
    with pytest.raises(NotImplementedError, match="text"):
        TA.score_latent_pairs_text(dd, z, z, z, z, None, "none", [2], 600)
    with pytest.raises(NotImplementedError, match="text"):
        TA.text_attention_maps(dd, z, z, None, "none", [2], 600)


def test_files_triplets_and_the_command_line(tiny, tmp_path, monkeypatch, capsys):
    from diffsim_amd import cli, harness as H, textattn as TA
    from diffsim_amd.inputs import path_latents
    from tests.test_gpu_regions import _image_files
    ds = _sd15(tiny, torch.float32)
    imgs = _image_files(tmp_path, 4, 1)
    # file entry == the latent call on path_latents' latents
    (latA, latB), nA, nB = path_latents(ds, [(imgs[0], imgs[1])], (0, 1), 128, 2334, 16)
    want = TA.score_latent_pairs_text(ds, latA, latB, nA, nB, "a cat", "up_blocks", 0, STEP, "cosine", words=["cat"], rel_threshold=1.1)
    got = ds.text_region_score(imgs[0], imgs[1], 128, "a cat", "up_blocks", [0], STEP, seed=2334, similarity="cosine", words=["cat"],
                               rel_threshold=1.1)
    assert got.shape == (1,) and torch.equal(got, want)
    m = ds.text_attention_map(imgs[0], imgs[1], 128, "a cat", "up_blocks", [0], STEP, seed=2334)
    assert m.shape[0] == 2 and m.shape[-1] == C.TINY.ctx_len
    # three triplets with a prompt per row == six pairwise calls, each with its row's prompt
    trip = [(imgs[0], imgs[1], imgs[2], "a cat"), (imgs[3], imgs[2], imgs[0], "the big dog"), (imgs[1], imgs[3], imgs[2], "a cat")]
    guide = TA.TextGuide()
    sl, sr, bad = H.score_path_triplets(ds, trip, 128, "up_blocks", [0], STEP, 2334, "cosine", batch_triplets=2, unet_triplets=2, text=guide)
    assert bad == 0 and 0.0 < guide.on_fraction < 1.0
    for i, t in enumerate(trip):
        wl = ds.text_region_score(t[0], t[1], 128, t[3], "up_blocks", [0], STEP, seed=2334, similarity="cosine")
        wr = ds.text_region_score(t[0], t[2], 128, t[3], "up_blocks", [0], STEP, seed=2334, similarity="cosine")
        assert torch.equal(wl[0], sl[i]) and torch.equal(wr[0], sr[i]), (i, wl, sl[i], wr, sr[i])
    plain = H.score_path_triplets(ds, trip, 128, "up_blocks", [0], STEP, 2334, "cosine", batch_triplets=2, unet_triplets=2)
    assert not torch.equal(plain[0], sl)
    with pytest.raises(ValueError):
        H.score_path_triplets(ds, trip, 128, "up_blocks", [0], STEP, 2334, "cosine", masks=[(None, None, None)] * 3, text=guide)
    # the command line over a tiny CUTE-shaped tree: class / instance / lighting / images
    from PIL import Image
    root = tmp_path / "cute"
    for inst in ("i0", "i1"):
        d = root / "cat" / inst / "light0"
        d.mkdir(parents=True)
        for j, src in enumerate(imgs[:2] if inst == "i0" else imgs[2:]):
            Image.open(src).save(d / f"{j}.png")
    cat_ctx = tiny["ctxs"][0]
    ds._ctx["The photo of a cat"] = cat_ctx.to(ds.device, torch.float32).contiguous()
    monkeypatch.setattr(cli, "build_scorer", lambda args: ds)
    rc = cli.main(["--dataset", "cute", "--image_path", str(root), "--image_size", "128", "--target_block", "up_blocks", "--target_layer", "0",
                   "--target_step", str(STEP), "--similarity", "cosine", "--text_attn", "cat", "--text_threshold", "1.0", "--batch", "4"])
    out = capsys.readouterr().out
    assert rc == 0 and "Text-guided regions: the words cat" in out and "Mean share of tokens on:" in out and "Total comparisons: 20" in out
    share = float(out.split("Mean share of tokens on:")[1].split("%")[0])
    assert 0.0 < share < 100.0
