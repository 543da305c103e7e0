"""End-to-end parity of the HIP scoring path (through the C ABI) against the CPU oracle and the
golden fixtures captured from the reference.  Gate (BASELINE.json north_star): scores within
1e-4 relative in the fp32 kernel mode on identical (latent, noise seed, timestep, weights);
the bf16 production mode reports its error against a looser, stated bound on the score; what the 16-bit walks compute tap by tap,
q / k / v against float64, is held in tests/test_gpu_walk64.py."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsim_amd import config as C
from diffsim_amd import synth as S

REL_F32 = 1e-4          # north_star tolerance, fp32 kernel mode
ABS_BF16 = 3e-2         # bf16 mode: absolute score error bound (scores live in [-1, 1])


@pytest.fixture(scope="module")
def tiny_env():
    from oracle import cpu_ref as R
    sd = S.make_state_dict(C.TINY, seed=0)
    return dict(sd=sd, oracle=R.build_unet(R.TINY, sd), ctx=S.make_context(C.TINY), R=R)


def _scorer(cfg, sd, dtype, **kw):
    from diffsim_amd.diffsim import DiffSim
    return DiffSim(torch_dtype=dtype, device="cuda", unet_config=cfg, state_dict=sd, **kw)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-6)


@pytest.mark.parametrize("block,layer,step", [("up_blocks", 0, 600), ("up_blocks", 1, 500), ("up_blocks", 2, 900),
                                              ("down_blocks", 0, 750), ("down_blocks", 1, 600),
                                              ("down_blocks", 2, 600), ("mid_blocks", 0, 900)])
def test_tiny_qkv_and_score_fp32(tiny_env, block, layer, step):
    R, unet, ctx = tiny_env["R"], tiny_env["oracle"], tiny_env["ctx"]
    ds = _scorer(C.TINY, tiny_env["sd"], torch.float32)
    zA, zB = S.make_pair_latents(C.TINY, 3)
    n = S.draw_pair_noise(2334, zA.shape)
    q, k, v = ds.features(torch.cat([zA, zB]), torch.cat([n[2], n[3]]), ctx, block, layer, step)
    for img, (z, nz) in enumerate(((zA, n[2]), (zB, n[3]))):
        qo, ko, vo = R.features(unet, z, nz, ctx, step, block, layer)
        for got, want in ((q, qo), (k, ko), (v, vo)):
            want = want.transpose(1, 2).reshape(2, want.shape[2], -1)       # (B,H,N,D) -> [B][N][H*D]
            err = (got[img].float().cpu() - want).abs().max().item()
            assert err <= 2e-4 * max(float(want.abs().max()), 1.0), (block, layer, err)
    for sim in ("cosine", "mse"):
        s = ds.diffsim_latents(zA, zB, n[2], n[3], ctx, block, layer, step, sim).cpu()
        so = R.diffsim_latents(unet, zA, zB, n[2], n[3], ctx, step, block, layer, sim)
        assert s.shape == (1,)
        assert _rel(float(s), float(so)) <= REL_F32, (sim, float(s), float(so))


def test_tiny_bf16_score_error(tiny_env):
    R, unet, ctx = tiny_env["R"], tiny_env["oracle"], tiny_env["ctx"]
    ds = _scorer(C.TINY, tiny_env["sd"], torch.bfloat16)
    errs = []
    for i in range(4):
        zA, zB = S.make_pair_latents(C.TINY, i)
        n = S.draw_pair_noise(2334, zA.shape)
        s = float(ds.diffsim_latents(zA, zB, n[2], n[3], ctx).cpu())
        so = float(R.diffsim_latents(unet, zA, zB, n[2], n[3], ctx))
        errs.append(abs(s - so))
    assert max(errs) <= ABS_BF16, errs


def test_golden_g5_reference_orchestration(tiny_env, golden_dir):
    """Scores the REFERENCE's DiffSim.diffsim + DiffSimPipeline.step produced (driving the oracle
    U-Net) must come out of the HIP path, both latents-in and through the path-based entry point
    with the shared fake VAE."""
    from tests._fakes import FakeVAE
    g = np.load(os.path.join(golden_dir, "g5_e2e_tiny.npz"))
    ctx = tiny_env["ctx"]
    ds = _scorer(C.TINY, tiny_env["sd"], torch.float32, vae=FakeVAE(), encode_prompt=lambda p: ctx)
    zA, zB, nA, nB = (torch.from_numpy(g[k]) for k in ("latA", "latB", "noiseA", "noiseB"))
    img_a, img_b = os.path.join(golden_dir, "g1_img_c.png"), os.path.join(golden_dir, "g1_img_d.png")
    for ci in range(6):
        blk, layer, step, sim = (str(x) for x in g[f"case_{ci}"])
        layer = json.loads(layer)
        if f"error_{ci}" in g.files:
            with pytest.raises(TypeError):
                ds.diffsim(img_a, img_b, 128, "The photo of a cat", blk, layer, int(step), seed=2334, similarity=sim)
            continue
        want = float(g[f"score_{ci}"][0])
        s_lat = float(ds.diffsim_latents(zA, zB, nA, nB, ctx, blk, layer, int(step), sim).cpu())
        s_path = ds.diffsim(img_a, img_b, 128, "The photo of a cat", blk, layer, int(step), seed=2334, similarity=sim)
        assert s_path.shape == (1,)
        assert _rel(s_lat, want) <= REL_F32, (ci, s_lat, want)
        assert _rel(float(s_path.cpu()), want) <= REL_F32, (ci, float(s_path.cpu()), want)
    # features of image B at the default tap against the reference's stored q/k/v
    q, k, v = ds.features(zB, nB, ctx, "up_blocks", 0, 600)
    for got, name in ((q, "qB"), (k, "kB"), (v, "vB")):
        want = torch.from_numpy(g[name]).transpose(1, 2).reshape(2, g[name].shape[2], -1)
        assert (got[0].float().cpu() - want).abs().max().item() <= 2e-4 * float(want.abs().max())


def test_batch_invariance_and_determinism(tiny_env):
    """batch-of-N == N singles bit for bit; same call twice is bit-identical."""
    ctx = tiny_env["ctx"]
    for dtype in (torch.float32, torch.bfloat16):
        ds = _scorer(C.TINY, tiny_env["sd"], dtype)
        lats = [S.make_pair_latents(C.TINY, i) for i in range(5)]
        zA = torch.cat([p[0] for p in lats])
        zB = torch.cat([p[1] for p in lats])
        n = S.draw_pair_noise(2334, lats[0][0].shape)
        s_all = ds.score_latent_pairs(zA, zB, n[2], n[3], ctx, batch_pairs=5)
        s_again = ds.score_latent_pairs(zA, zB, n[2], n[3], ctx, batch_pairs=5)
        s_split = ds.score_latent_pairs(zA, zB, n[2], n[3], ctx, batch_pairs=2)
        assert torch.equal(s_all, s_again)
        assert torch.equal(s_all, s_split)
        for i in range(5):
            s1 = ds.diffsim_latents(zA[i:i + 1], zB[i:i + 1], n[2], n[3], ctx)
            assert torch.equal(s1[0], s_all[i])
        assert float(s_all.min()) >= -1.0 and float(s_all.max()) <= 1.0


def test_hipgraph_replay_is_bit_identical(tiny_env):
    """use_graphs=True replays the captured forward; scores must equal the eager launches bit for bit, also after
    new inputs are copied into the static buffers and after a timestep change invalidates the graphs."""
    ctx = tiny_env["ctx"]
    eager = _scorer(C.TINY, tiny_env["sd"], torch.bfloat16)
    graph = _scorer(C.TINY, tiny_env["sd"], torch.bfloat16, use_graphs=True)
    n = S.draw_pair_noise(2334, (1, 4, C.TINY.sample_size, C.TINY.sample_size))
    for step in (600, 600, 750):
        for i in range(3):
            zA, zB = S.make_pair_latents(C.TINY, i)
            a = eager.score_latent_pairs(zA, zB, n[2], n[3], ctx, "up_blocks", 0, step)
            b = graph.score_latent_pairs(zA, zB, n[2], n[3], ctx, "up_blocks", 0, step)
            assert torch.equal(a, b)
    assert len(graph.engine("up_blocks", 0)._graphs) == 1


def test_properties_slot_noise(tiny_env):
    ctx = tiny_env["ctx"]
    ds = _scorer(C.TINY, tiny_env["sd"], torch.float32)
    zA, zB = S.make_pair_latents(C.TINY, 0)
    n = S.draw_pair_noise(2334, zA.shape)
    s_ab = float(ds.diffsim_latents(zA, zB, n[2], n[3], ctx).cpu())
    s_aa = float(ds.diffsim_latents(zA, zA, n[2], n[3], ctx).cpu())
    s_swap = float(ds.diffsim_latents(zB, zA, n[3], n[2], ctx).cpu())
    assert s_aa < 1.0                               # slot-dependent noise: diffsim(A,A) != 1
    assert abs(s_ab - s_swap) < 1e-6                # swapping images AND their noise is symmetric
    s_same = float(ds.diffsim_latents(zA, zA, n[2], n[2], ctx).cpu())
    assert abs(s_same - 1.0) < 1e-5                 # identical latents AND noise -> exactly similar


def test_sd15_channels_small_latent_fp32():
    """Real SD1.5 channel plan (320/640/1280, 8 heads x 40/80/160, 77x768 context, 2560/1920-ch concat
    GroupNorms) on an 8x8 latent: every kernel shape family of config 1, oracle in seconds."""
    from oracle import cpu_ref as R
    cfg = C.SD15_SMALL
    keys = [k for k in C.unet_param_shapes(cfg) if not k.startswith(("up_blocks.2", "up_blocks.3", "conv_norm_out",
                                                                      "conv_out"))]
    sd = S.make_state_dict(cfg, seed=0, keys=keys)
    full = dict(sd)
    for k, shp in C.unet_param_shapes(cfg).items():      # oracle wants every key; the rest is unused
        if k not in full:
            full[k] = torch.zeros(shp)
    rcfg = R.UNetConfig(sample_size=8)
    unet = R.build_unet(rcfg, full)
    ctx = S.make_context(cfg)
    ds = _scorer(cfg, sd, torch.float32)
    dsb = _scorer(cfg, sd, torch.bfloat16)
    for i in range(2):
        zA, zB = S.make_pair_latents(cfg, i)
        n = S.draw_pair_noise(2334, zA.shape)
        so = float(R.diffsim_latents(unet, zA, zB, n[2], n[3], ctx))
        s = float(ds.diffsim_latents(zA, zB, n[2], n[3], ctx).cpu())
        assert _rel(s, so) <= REL_F32, (s, so)
        sb = float(dsb.diffsim_latents(zA, zB, n[2], n[3], ctx).cpu())
        assert abs(sb - so) <= ABS_BF16, (sb, so)


def test_errors_are_loud(tiny_env, golden_dir):
    from diffsim_amd import _lib
    ds = _scorer(C.TINY, tiny_env["sd"], torch.float32)
    img = os.path.join(golden_dir, "g1_img_c.png")
    with pytest.raises(RuntimeError):
        ds.diffsim(img, img, 128, "p", "up_blocks", [0], 600)                   # no VAE plugged in
    with pytest.raises(IndexError):
        zA, zB = S.make_pair_latents(C.TINY, 0)
        ds.diffsim_latents(zA, zB, zA, zB, tiny_env["ctx"], target_step=0)      # idx 0 -> t=1000
    with pytest.raises(_lib.DsimError):
        from diffsim_amd.engine import UNetEngine
        UNetEngine(C.TINY, {"conv_in.weight": tiny_env["sd"]["conv_in.weight"]}, torch.float32)   # missing weights


def test_triplet_harness_matches_pairwise_calls(tiny_env, golden_dir, tmp_path):
    """NIGHTS-shaped 2AFC run (config 3 shape): cached-reference triplet scoring must reproduce,
    bit for bit, the two separate scorer calls per triplet the reference driver makes
    (night_main.py:69-163), and the accuracy rule must match."""
    import csv
    import shutil
    from diffsim_amd import harness as Hn
    from tests._fakes import FakeVAE
    ctx = tiny_env["ctx"]
    ds = _scorer(C.TINY, tiny_env["sd"], torch.float32, vae=FakeVAE(), encode_prompt=lambda p: ctx)
    names = ["g1_img_a.png", "g1_img_b.png", "g1_img_c.png", "g1_img_d.png"]
    for n in names:
        shutil.copy(os.path.join(golden_dir, n), tmp_path / n)
    rows = [("val", names[0], names[1], names[2], 1, "Cat"), ("train", names[1], names[2], names[3], 0, "Dog"),
            ("val", names[3], names[0], names[1], 0, "Dog"), ("val", names[2], names[3], names[0], 1, "Cat")]
    with open(tmp_path / "data.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["split", "ref_path", "left_path", "right_path", "left_vote", "prompt"])
        w.writerows(rows)
    parsed = Hn.read_nights_csv(str(tmp_path))
    assert len(parsed) == 3 and parsed[0]["prompt"] == "An image of a cat"
    for sim in ("cosine", "mse"):
        acc = Hn.nights_eval(ds, str(tmp_path), 128, "up_blocks", [0], 600, seed=2334, similarity=sim)
        correct = 0
        for r in parsed:
            ab = ds.diffsim(r["ref"], r["left"], 128, r["prompt"], "up_blocks", [0], 600, seed=2334, similarity=sim)
            ac = ds.diffsim(r["ref"], r["right"], 128, r["prompt"], "up_blocks", [0], 600, seed=2334, similarity=sim)
            pred = (1 if ab < ac else 0) if sim == "mse" else (1 if ab > ac else 0)
            correct += int(pred == r["vote"])
        assert abs(acc - 100.0 * correct / len(parsed)) < 1e-3
    # the same run with the HIP VAE encoder (chunked encodes, threaded decode): same rule, same accuracy as pairwise calls
    from diffsim_amd.engine import VAEEncoder
    dv = _scorer(C.TINY, tiny_env["sd"], torch.float32, vae=VAEEncoder(C.VAE_TINY, S.make_state_dict(C.VAE_TINY, seed=3), torch.float32),
                 encode_prompt=lambda p: ctx)
    acc = Hn.nights_eval(dv, str(tmp_path), 128, "up_blocks", [0], 600, seed=2334, similarity="cosine", batch_triplets=2)
    correct = 0
    for r in parsed:
        ab = dv.diffsim(r["ref"], r["left"], 128, r["prompt"], "up_blocks", [0], 600, seed=2334, similarity="cosine")
        ac = dv.diffsim(r["ref"], r["right"], 128, r["prompt"], "up_blocks", [0], 600, seed=2334, similarity="cosine")
        correct += int((1 if ab > ac else 0) == r["vote"])
    assert abs(acc - 100.0 * correct / len(parsed)) < 1e-3
    # bit-exact equality of cached-reference scores with the pairwise path
    lat = [S.make_pair_latents(C.TINY, i) for i in range(3)]
    ref = torch.cat([p[0] for p in lat]); left = torch.cat([p[1] for p in lat]); right = torch.cat([p[0] for p in lat[::-1]])
    n = S.draw_pair_noise(2334, lat[0][0].shape)
    sl, sr = Hn.score_latent_triplets(ds, ref, left, right, n[2], n[3], ctx, batch_triplets=2)
    pl = ds.score_latent_pairs(ref, left, n[2], n[3], ctx)
    pr = ds.score_latent_pairs(ref, right, n[2], n[3], ctx)
    assert torch.equal(sl, pl) and torch.equal(sr, pr)


def test_sd15_full_size_fp32_and_bf16_pairs():
    """BASELINE config 1 shape: the real SD1.5 graph at 512 px (64x64 latents, 256-token tap, 8 heads x 160),
    synthetic pairs, fp32 kernel mode vs the fp32 CPU oracle at the north_star tolerance (1e-4 relative), and
    the bf16 production mode's error on the same pairs."""
    from oracle import cpu_ref as R
    cfg = C.SD15
    keys = [k for k in C.unet_param_shapes(cfg) if not k.startswith(("up_blocks.2", "up_blocks.3", "conv_norm_out", "conv_out"))]
    sd = S.make_state_dict(cfg, seed=0, keys=keys)
    full = dict(sd)
    for k, shp in C.unet_param_shapes(cfg).items():
        if k not in full:
            full[k] = torch.zeros(shp)
    unet = R.build_unet(R.SD15, full)
    del full
    ctx = S.make_context(cfg)
    n = S.draw_pair_noise(2334, (1, 4, 64, 64))
    lats = [S.make_pair_latents(cfg, i) for i in range(2)]
    want = [float(R.diffsim_latents(unet, a, b, n[2], n[3], ctx)) for a, b in lats]
    zA = torch.cat([p[0] for p in lats]); zB = torch.cat([p[1] for p in lats])
    got32 = _scorer(cfg, sd, torch.float32).score_latent_pairs(zA, zB, n[2], n[3], ctx).cpu()
    for s, w in zip(got32.tolist(), want):
        assert _rel(s, w) <= REL_F32, (s, w)
    sc16 = _scorer(cfg, sd, torch.bfloat16)
    got16 = sc16.score_latent_pairs(zA, zB, n[2], n[3], ctx).cpu()
    for s, w in zip(got16.tolist(), want):
        assert abs(s - w) <= 5e-3, (s, w)
    # the 2 GiB-per-tensor bound of the 32-bit buffer offsets: the planner reports it, qkv refuses it loudly
    from diffsim_amd import _lib
    eng = sc16.engine("up_blocks", 0)
    mx = eng.max_images()
    assert 64 <= mx < 512 and eng.workspace_bytes(mx) > 0 and eng.workspace_bytes(mx + 1) == 0
    big = torch.zeros(mx + 1, 4, 64, 64, device="cuda")
    with pytest.raises(_lib.DsimError):
        eng.qkv(big, big, 1.0, 0.0, ctx.cuda())


def test_batch_is_split_at_the_2gib_tensor_bound(tiny_env):
    """workspace_bytes() is 0 for a batch whose activations would reach 2 GiB; qkv() refuses it loudly and
    score_latent_pairs() splits the batch instead (same scores as small batches)."""
    from diffsim_amd import _lib
    ds = _scorer(C.TINY, tiny_env["sd"], torch.bfloat16)
    eng = ds.engine("up_blocks", 0)
    mx = eng.max_images()
    assert mx >= 2 and eng.workspace_bytes(mx) > 0
    if mx < 4096:
        assert eng.workspace_bytes(mx + 1) == 0
