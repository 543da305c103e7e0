"""Similarity maps (dsim_pair_score_maps / engine.pair_score_maps / maps.py / the scorers' similarity_maps): the score tail kept
per query token.  Checked against the reference's tail arithmetic restated per token in float64 torch
(/root/reference/diffsim/diffsim.py:177-197, as test_gpu_matrix._tail64), against the pair path on the same features, against
the golden tail, and end to end against score_latent_pairs / diffsim."""
import os

import numpy as np
import pytest
import torch

from tests._tail64 import pairs64

pytestmark = pytest.mark.gpu

B = 2


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


def _maps64(q, k, v, ia, ib, H, sim, out_dtype):
    """Per pair: score, local (2, N), contrib (2, N) in float64 -- float64 SDPAs on the rounded operands, their outputs rounded to
    the pipeline dtype, then the per-token terms of cosine / mse (tests/_tail64.py)"""
    return pairs64(q, k, v, ia.cpu(), ib.cpu(), H, sim, out_dtype)


def _feats(n, seed, dtype, N, H, D, logit_scale=1.0, correlate=0.5):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(n, B, N, H * D, generator=g) for _ in range(3))
    base = tuple(torch.randn(1, B, N, H * D, generator=g) for _ in range(3))
    q, k, v = (correlate * b + (1 - correlate) * t for b, t in zip(base, (q, k, v)))
    q = q * logit_scale
    return tuple(t.to(dtype).cuda().contiguous() for t in (q, k, v))


def _idx(*xs):
    return torch.tensor(list(xs), dtype=torch.int32).cuda()


def _score_tol(dtype, peaked):
    if dtype == torch.float32:
        return 1e-5
    if peaked:                  # (test_gpu_round6's peaked-logit tolerances of the pair tail)
        return 1e-2 if dtype == torch.bfloat16 else 2e-3
    return 4e-3 if dtype == torch.bfloat16 else 5e-4


def _score_err(got, want, sim, dtype):
    """cosine: absolute (relative in fp32); mse: relative"""
    if sim == "cosine" and dtype != torch.float32:
        return abs(got - want)
    return abs(got - want) / max(abs(want), 1e-6)


# 16-bit local-map gates: 4 x the largest error of the first MI355X run (similarity maps)
# (observed maxima: bf16 cosine 1.88e-3, fp16 cosine 1.68e-4 absolute; bf16 mse 3.63e-3, fp16 mse 3.86e-4 relative)
LOCAL_GATE = {(torch.bfloat16, "cosine"): 7.5e-3, (torch.float16, "cosine"): 6.7e-4,
              (torch.bfloat16, "mse"): 1.45e-2, (torch.float16, "mse"): 1.5e-3}
LOCAL_LOG = os.environ.get("DSIM_MAPS_LOCAL_LOG")


def _local_err(got, want, sim):
    if sim == "cosine":
        return (got - want).abs().max().item()
    return ((got - want).abs() / want.abs().clamp_min(1e-3)).max().item()


SHAPES = [(torch.bfloat16, 256, 8, 160), (torch.float16, 256, 8, 160), (torch.float32, 256, 8, 160),
          (torch.bfloat16, 1024, 8, 80), (torch.float16, 1024, 8, 80), (torch.float32, 1024, 8, 80),
          (torch.bfloat16, 256, 16, 72), (torch.float32, 256, 16, 72),
          (torch.float16, 1024, 20, 64), (torch.float32, 1024, 20, 64),
          (torch.bfloat16, 64, 4, 32), (torch.float32, 64, 4, 32)]


@pytest.mark.parametrize("dtype,N,H,D", SHAPES)
@pytest.mark.parametrize("sim", ["cosine", "mse"])
@pytest.mark.parametrize("peaked", [False, True])
def test_maps_match_float64_the_pair_path_and_sum_to_the_score(eng, dtype, N, H, D, sim, peaked):
    scale = 14.0 if peaked else 1.0
    q, k, v = _feats(4, 11 + N + D, dtype, N, H, D, logit_scale=scale)
    ia, ib = _idx(0, 2, 3), _idx(1, 0, 1)
    score, local, contrib = eng.pair_score_maps(q, k, v, ia, ib, H, sim)
    assert score.shape == (3,) and local.shape == (3, 2, N) and contrib.shape == (3, 2, N)
    assert all(t.dtype == torch.float32 and t.is_cuda for t in (score, local, contrib))
    want = _maps64(q, k, v, ia, ib, H, sim, dtype)
    tol = _score_tol(dtype, peaked)
    for p, (ws, wl, wc) in enumerate(want):
        gs = float(score[p])
        # 1. against the float64 restatement
        assert _score_err(gs, ws, sim, dtype) <= (tol if sim == "cosine" else 10 * tol), (p, gs, ws)
        gl = local[p].double().cpu()
        err = _local_err(gl, wl, sim)
        if LOCAL_LOG:
            with open(LOCAL_LOG, "a") as f:
                f.write(f"{str(dtype)[6:]} {sim} N={N} H={H} D={D} peaked={peaked} local_err={err:.3e}\n")
        if dtype == torch.float32:
            assert (gl - wl).abs().max().item() <= 1e-5, (p, (gl - wl).abs().max().item())
        else:
            assert err <= LOCAL_GATE[(dtype, sim)], (p, err)
        # 2. the maps sum to the score
        total = 0.5 * contrib[p].double().sum().item()
        assert abs(total - gs) <= 1e-6 * max(1.0, abs(gs)), (p, total, gs)
    # 3. agreement with the pair path (the same attend and products; at the default tap the 16-bit pair path is the persistent kernel)
    ps = eng.pair_score(q, k, v, ia, ib, H, sim)
    default_tap_16 = dtype != torch.float32 and (N, D) == (256, 160)
    for p, (ws, _, _) in enumerate(want):
        if default_tap_16:
            assert _score_err(float(ps[p]), ws, sim, dtype) <= (tol if sim == "cosine" else 10 * tol)
        else:
            assert abs(float(score[p]) - float(ps[p])) <= 1e-6 * max(1.0, abs(float(ps[p]))), (p, float(score[p]), float(ps[p]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_maps_score_the_golden_tail(eng, dtype, golden_dir):
    """tests/golden/g4_tail.npz (the reference's own tail): test_gpu_ops' cases and tolerances, through pair_score_maps."""
    g4 = np.load(os.path.join(golden_dir, "g4_tail.npz"))
    for i in range(10):
        shp = tuple(int(x) for x in g4[f"shape_{i}"])
        gen = torch.Generator("cpu").manual_seed(int(g4[f"seed_{i}"][0]))
        sets = [[torch.randn(shp, generator=gen) * (1.5 if j == 0 else 1.0) for j in range(3)] for _ in range(2)]
        mixw = 0.3 + 0.07 * i
        sets[1] = [mixw * a + (1 - mixw) * b for a, b in zip(sets[0], sets[1])]
        if i == 8:
            sets[1] = [t.clone() for t in sets[0]]
        Bc, H, N, D = shp
        feats = [torch.stack([s[j].transpose(1, 2).reshape(Bc, N, H * D) for s in sets]) for j in range(3)]
        q, k, v = (f.cuda().to(dtype).contiguous() for f in feats)
        for sim in ("cosine", "mse"):
            got = float(eng.pair_score_maps(q, k, v, _idx(0), _idx(1), H, sim)[0][0])
            want = float(g4[f"score_{i}_{sim}"][0])
            tol = 1e-4 if dtype == torch.float32 else 3e-2
            assert abs(got - want) <= tol * max(abs(want), 1e-2), (i, sim, got, want)


@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float16, 256, 8, 160), (torch.float32, 256, 8, 160),
                                         (torch.bfloat16, 1024, 8, 80), (torch.float32, 256, 16, 72)])
def test_self_pairs(eng, dtype, N, H, D):
    """An image against itself: cosine local 1 at every token, mse maps 0.  (The self and the cross attention are two inlined
    copies of attend, as in pair_tail_kernel, and may round the last bit differently: mse is 0 to within 1e-8, not exactly.)"""
    q, k, v = _feats(3, 5, dtype, N, H, D)
    ia = _idx(0, 1, 2)
    s, lo, co = eng.pair_score_maps(q, k, v, ia, ia, H, "cosine")
    assert lo.min().item() >= 1 - 1e-6, lo.min().item()
    assert (s - 1).abs().max().item() <= 1e-6
    s, lo, co = eng.pair_score_maps(q, k, v, ia, ia, H, "mse")
    for t in (s, lo, co):
        assert t.min().item() >= 0 and t.max().item() <= 1e-8, (t.min().item(), t.max().item())


@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float16, 1024, 8, 80), (torch.float32, 256, 16, 72)])
def test_reproducible_batch_invariant_and_swap_symmetric(eng, dtype, N, H, D):
    q, k, v = _feats(12, 7, dtype, N, H, D)
    g = torch.Generator().manual_seed(3)
    ia = torch.randint(0, 12, (64,), generator=g, dtype=torch.int32).cuda()
    ib = torch.randint(0, 12, (64,), generator=g, dtype=torch.int32).cuda()
    for sim in ("cosine", "mse"):
        r1 = eng.pair_score_maps(q, k, v, ia, ib, H, sim)
        r2 = eng.pair_score_maps(q, k, v, ia, ib, H, sim)
        assert all(torch.equal(a, b) for a, b in zip(r1, r2))
        for p in (0, 17, 63):                       # a pair alone == the same pair inside the batch of 64
            one = eng.pair_score_maps(q, k, v, ia[p:p + 1].clone(), ib[p:p + 1].clone(), H, sim)
            assert all(torch.equal(a[0], b[p]) for a, b in zip(one, r1))
        sw = eng.pair_score_maps(q, k, v, ib, ia, H, sim)           # swapping (a, b) swaps the directions
        assert torch.equal(sw[0], r1[0])
        assert torch.equal(sw[1], r1[1].flip(1)) and torch.equal(sw[2], r1[2].flip(1))


@pytest.mark.parametrize("dtype,N,H,D", [(torch.float16, 256, 8, 160), (torch.bfloat16, 1024, 8, 80), (torch.float32, 256, 8, 160)])
def test_non_finite_pair_is_flagged_and_leaves_the_others(eng, dtype, N, H, D):
    q, k, v = _feats(4, 9, dtype, N, H, D)
    ia, ib = _idx(0, 1, 2), _idx(1, 2, 3)
    clean = eng.pair_score_maps(q, k, v, ia, ib, H, "cosine", return_status=True)
    assert clean[3].tolist() == [0, 0, 0]
    k2 = k.clone()
    k2[3, 1, 17, 5] = float("inf")
    s, lo, co, st = eng.pair_score_maps(q, k2, v, ia, ib, H, "cosine", return_status=True)
    assert st.tolist() == [0, 0, 1]
    for a, b in zip((s, lo, co), clean[:3]):
        assert torch.equal(a[:2], b[:2])


def test_invalid_arguments(eng):
    from diffsim_amd import _lib
    q, k, v = _feats(2, 1, torch.bfloat16, 64, 4, 32)
    with pytest.raises(_lib.DsimError):
        eng.pair_score_maps(q, k.float(), v, _idx(0), _idx(1), 4)
    with pytest.raises(_lib.DsimError):
        eng.pair_score_maps(q, k, v, _idx(0), _idx(1), 5)
    L = _lib.lib()
    assert L.dsim_pair_score_maps_workspace_bytes(0, 2, 4, 64, 32) == 0
    need = L.dsim_pair_score_maps_workspace_bytes(1, 2, 4, 64, 32)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty(1, device="cuda")
    ia, ib = _idx(0), _idx(1)
    args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), ia.data_ptr(), ib.data_ptr(), 1, 2, 4, 64, 32, _lib.DSIM_BF16, 0,
            out.data_ptr(), None, None, None)
    rc = L.dsim_pair_score_maps(*args, ws.data_ptr(), need // 2, None)
    assert rc != 0 and b"workspace" in L.dsim_strerror(rc).lower()
    assert L.dsim_pair_score_maps(*args, ws.data_ptr(), need, None) == 0          # local / contrib / status may be NULL
    torch.cuda.synchronize()
    ref = eng.pair_score_maps(q, k, v, ia, ib, 4)[0]
    assert torch.equal(out, ref)
    big = torch.zeros(32768, dtype=torch.int32, device="cuda")
    assert L.dsim_pair_score_maps(q.data_ptr(), k.data_ptr(), v.data_ptr(), big.data_ptr(), big.data_ptr(), 32768, 2, 4, 64, 32,
                                  _lib.DSIM_BF16, 0, out.data_ptr(), None, None, None, ws.data_ptr(), 1 << 62, None) != 0


# ---- end to end on synthetic weights ------------------------------------------------------------------------------------------
def test_sd15_512px_latent_pair_maps_match_score_latent_pairs():
    """fp32 at SD1.5's full size: the maps' scores equal score_latent_pairs' within 1e-6, on the taps' grids."""
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim import DiffSim
    cfg = C.SD15
    sd = S.make_state_dict(cfg, seed=0)
    ctx = S.make_context(cfg)
    n = S.draw_pair_noise(2334, (1, 4, 64, 64))
    lat = [S.make_pair_latents(cfg, i) for i in range(3)]
    la = torch.cat([p[0] for p in lat])
    lb = torch.cat([lat[0][1], lat[1][1], lat[0][0]])            # (the third pair: an image against itself)
    ds = DiffSim(torch_dtype=torch.float32, device="cuda", unet_config=cfg, state_dict=sd)
    for block, layer, grid in (("up_blocks", 0, (16, 16)), ("up_blocks", 1, (32, 32)), ("mid_blocks", 0, (8, 8))):
        for sim in ("cosine", "mse"):
            m = ds.score_latent_pair_maps(la, lb, n[2], n[3], ctx, block, layer, 600, sim)
            p = ds.score_latent_pairs(la, lb, n[2], n[3], ctx, block, layer, 600, sim)
            assert m.grid == grid and m.local.shape == (3, 2) + grid
            assert ((m.score - p).abs() <= 1e-6 * p.abs().clamp_min(1.0)).all(), (block, layer, sim, m.score, p)
            assert abs(0.5 * m.contrib[0].double().sum().item() - float(m.score[0])) <= 1e-6 * max(1.0, abs(float(m.score[0])))


def _image_files(tmp_path, n, seed):
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    paths = []
    for i in range(n):
        base = torch.rand(3, 1, 1, generator=g) * 255
        px = (base + 60 * torch.randn(3, 160, 144, generator=g)).clamp(0, 255).to(torch.uint8)
        p = tmp_path / f"img{seed}_{i}.png"
        Image.fromarray(px.permute(1, 2, 0).numpy()).save(p)
        paths.append(str(p))
    return paths


def _close(a, b, rel=1e-5):
    a, b = float(a), float(b)
    assert abs(a - b) <= rel * max(abs(b), 1e-6), (a, b)


def test_sd15_similarity_maps_match_diffsim_on_image_files(tmp_path):
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.engine import VAEEncoder
    from diffsim_amd.maps import score_path_pair_maps
    ctx = S.make_context(C.TINY)
    vae = VAEEncoder(C.VAE_TINY, S.make_state_dict(C.VAE_TINY, seed=3), torch.float32)
    ds = DiffSim(torch_dtype=torch.float32, device="cuda", unet_config=C.TINY, state_dict=S.make_state_dict(C.TINY, seed=0),
                 vae=vae, encode_prompt=lambda p: ctx)
    a, b, c = _image_files(tmp_path, 3, 1)
    for sim in ("cosine", "mse"):
        m = ds.similarity_maps(a, b, 128, "a cat", "up_blocks", [0], 600, seed=2334, similarity=sim)
        assert len(m) == 1 and m.local.shape[:2] == (1, 2) and m.grid[0] == m.grid[1]
        _close(m.score[0], ds.diffsim(a, b, 128, "a cat", "up_blocks", [0], 600, seed=2334, similarity=sim))
    pm = score_path_pair_maps(ds, [(a, b), (a, c)], 128, "a cat", "up_blocks", 0, 600, 2334, "cosine")
    want = ds.score_pairs([(a, b), (a, c)], 128, "a cat", "up_blocks", 0, 600, seed=2334, similarity="cosine")
    assert (pm.score - want).abs().max().item() <= 1e-6


def test_dit_similarity_maps(tmp_path):
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim_dit import diffsim_DiT
    from tests._fakes import FakeVAE
    dd = diffsim_DiT(128, 600, "cuda", dit_config=C.DIT_TINY, state_dict=S.make_state_dict(C.DIT_TINY, seed=0), vae=FakeVAE(),
                     torch_dtype=torch.float32)
    a, b = _image_files(tmp_path, 2, 7)
    m = dd.similarity_maps(a, b, 128, "p", "none", [2], 600, "cosine", 2334)
    side = C.DIT_TINY.input_size // C.DIT_TINY.patch_size
    assert m.grid == (side, side) and m.local.shape == (1, 2, side, side)
    _close(m.score[0], dd.diffsim_score(a, b, 128, "p", "none", [2], 600, "cosine", 2334).reshape(-1)[0])


def test_xl_similarity_maps(tmp_path):
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim_xl import diffsim_xl
    from tests._fakes import FakeVAE
    ctx, pooled = S.make_context(C.SDXL_TINY), S.make_pooled(C.SDXL_TINY)
    xl = diffsim_xl(torch.float32, "cuda", unet_config=C.SDXL_TINY, state_dict=S.make_state_dict(C.SDXL_TINY, seed=0), vae=FakeVAE(),
                    encode_prompt=lambda p: (ctx, pooled))
    a, b = _image_files(tmp_path, 2, 5)
    for sim in ("cosine", "mse"):
        m = xl.similarity_maps(a, b, 128, "a cat", "up_blocks", [0, 1, 2], 600, sim, 2334)
        assert m.grid[0] == m.grid[1] and m.local.shape[:2] == (1, 2)
        _close(m.score[0], xl.diffsim_score(a, b, 128, "a cat", "up_blocks", [0, 1, 2], 600, sim, 2334).reshape(-1)[0])


def test_cli_save_maps_writes_one_npz_per_query(tmp_path, monkeypatch):
    """--dataset retrieval --save_maps on a tiny generated gallery: one .npz per query beside its ranking, the stated shapes, and
    the scores of the ranking file (fp32)."""
    from diffsim_amd import cli, config as C, synth as S
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.engine import VAEEncoder
    ctx = S.make_context(C.TINY)
    vae = VAEEncoder(C.VAE_TINY, S.make_state_dict(C.VAE_TINY, seed=3), torch.float32)
    ds = DiffSim(torch_dtype=torch.float32, device="cuda", unet_config=C.TINY, state_dict=S.make_state_dict(C.TINY, seed=0),
                 vae=vae, encode_prompt=lambda p: ctx)
    qdir, gdir, out = tmp_path / "q", tmp_path / "g", tmp_path / "out"
    qdir.mkdir(), gdir.mkdir()
    _image_files(qdir, 2, 11), _image_files(gdir, 4, 12)
    monkeypatch.setattr(cli, "build_scorer", lambda args: ds)
    args = cli.arg_parse(["--dataset", "retrieval", "--query_path", str(qdir), "--image_path", str(gdir), "--out_path", str(out),
                          "--image_size", "128", "--target_block", "up_blocks", "--target_layer", "0", "--target_step", "600",
                          "--similarity", "cosine", "--topk", "3", "--save_maps"])
    assert cli.run(args) == 0
    for name in ("img11_0", "img11_1"):
        rank = [l.split() for l in open(out / f"{name}.txt").read().splitlines()]
        z = np.load(out / f"{name}.npz")
        k = len(rank)
        assert k == 3 and z["gallery"].tolist() == [r[0] for r in rank]
        h = z["local"].shape[2]
        assert z["score"].shape == (k,) and z["local"].shape == (k, 2, h, h) and z["contrib"].shape == (k, 2, h, h)
        for s, r in zip(z["score"].tolist(), rank):
            assert abs(s - float(r[1])) <= 1e-6 * max(1.0, abs(float(r[1]))), (s, r)
        assert np.allclose(0.5 * z["contrib"].astype(np.float64).sum((1, 2, 3)), z["score"], rtol=0, atol=1e-6)
