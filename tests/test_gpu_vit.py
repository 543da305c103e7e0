"""clip_cross / dino_cross on the GPU: the ViT executor (csrc/vit.hip), the projected score tail (csrc/tail_proj.hip) and the scorers
(diffsim_amd/vit.py) against the float64 restatement tests/_vit64.py, which tests/test_vit_host.py pins to transformers and to the
reference's own tails.

Tolerances are the project's: fp32 scores 1e-4 relative (the parity gate), fp32 q/k/v 2e-4 max|ref| (tests/test_gpu_dit.py:44), bf16 /
fp16 scores 3e-2 absolute (tests/test_gpu_dit.py:39).  Shapes: tiny configs (C 128, 2 x 64 heads, depth 3, patch 8); side 40 gives
N = 26 (no multiple of 16), side 128 N = 257 (three 128-query tiles, the last of one row); 1 and 3 images give ragged GEMM rows.
Measured maxima stand beside the 16-bit assertions.
"""
import dataclasses
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsim_amd import _lib, config as C, synth as S
from tests import _vit64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
IMGS = [os.path.join(GOLDEN, f"g1_img_{c}.png") for c in "abcd"]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _cfg(kind, side):
    base = C.VIT_TINY_CLIP if kind == "clip" else C.VIT_TINY_DINO
    if kind == "clip" and side != base.image_size:          # CLIP has one side: a tower whose stored table is that side's
        return dataclasses.replace(base, image_size=side, pos_grid=side // base.patch_size)
    return base


def _pixels(n, side, seed=5):
    return torch.randn(n, 3, side, side, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def weights():
    return {(k, s): S.make_state_dict(_cfg(k, s), 3) for k in ("clip", "dinov2") for s in (40, 128)}


# ---- 1. the executor ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [40, 128])
@pytest.mark.parametrize("kind", ["clip", "dinov2"])
def test_qkv_fp32_against_float64_at_every_tap(kind, side, weights):
    from diffsim_amd.engine import ViTEngine
    cfg, sd = _cfg(kind, side), weights[(kind, side)]
    eng = ViTEngine(cfg, sd, torch.float32, 0, "cuda:0", side)
    handle = eng._h.value
    x3 = _pixels(3, side)
    single = {}
    for n, x in ((3, x3), (1, x3[1:2])):
        for L in (0, 1, 2):
            eng.set_tap(L)
            assert eng._h.value == handle                    # the tap moved, the packed weights stayed
            got = eng.qkv(x.cuda())
            for g, w in zip(got, R.tap_qkv(sd, cfg, x, L)):
                assert g.shape == (n, 1, cfg.tokens(side), cfg.hidden_size)
                err = (g[:, 0].double().cpu() - w).abs().max().item()
                assert err <= 2e-4 * float(w.abs().max()), (kind, side, n, L, err)
            if n == 3:
                single[L] = got
    # one walk for three taps, any order: bit for bit the one-tap calls; the handle's tap does not move
    eng.set_tap(1)
    sweep = eng.qkv_taps(x3.cuda(), [0, 2, 1])
    for L, got in zip([0, 2, 1], sweep):
        assert all(torch.equal(a, b) for a, b in zip(got, single[L])), L
    assert eng.target_layer == 1 and all(torch.equal(a, b) for a, b in zip(eng.qkv(x3.cuda()), single[1]))
    # a handle created at tap 2 gives what the moved tap gives
    fresh = ViTEngine(cfg, sd, torch.float32, 2, "cuda:0", side)
    assert all(torch.equal(a, b) for a, b in zip(fresh.qkv(x3.cuda()), single[2]))
    for bad in ([0, 0], [3], []):
        with pytest.raises(_lib.DsimError):
            eng.qkv_taps(x3.cuda(), bad)


def test_vit_handle_refusals(weights):
    from diffsim_amd.engine import ViTEngine
    cfg, sd = _cfg("dinov2", 40), weights[("dinov2", 40)]
    with pytest.raises(_lib.DsimError, match="dsim_vit_create"):
        ViTEngine(cfg, sd, torch.float32, 3, "cuda:0")                    # tap outside [0, depth)
    with pytest.raises(_lib.DsimError, match="finalize"):                  # a block before the tap was never loaded
        ViTEngine(cfg, {k: v for k, v in sd.items() if not k.startswith("blocks.1.norm1")}, torch.float32, 2, "cuda:0")
    with pytest.raises(_lib.DsimError, match="no interpolation"):
        ViTEngine(_cfg("clip", 40), weights[("clip", 40)], torch.float32, 0, "cuda:0", 48)
    part = ViTEngine(cfg, {k: v for k, v in sd.items() if not k.startswith("blocks.2.")}, torch.float32, 1, "cuda:0")
    with pytest.raises(_lib.DsimError, match="set_tap"):
        part.set_tap(2)
    assert part.target_layer == 1
    with pytest.raises(_lib.DsimError, match="float32"):
        part.qkv(_pixels(1, 48).cuda())


# ---- 2. pair scores through the scorers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("kind", ["dinov2", "clip"])
def test_pair_scores_against_float64(kind, dtype, weights):
    """score_pixel_pairs at every layer and both sides.  Measured maxima of |score - float64| (MI355X): see the assertion."""
    from diffsim_amd.vit import CLIPScore, Dinov2Score
    worst = 0.0
    for side in (40, 128):
        cfg, sd = _cfg(kind, side), weights[(kind, side)]
        sc = (CLIPScore if kind == "clip" else Dinov2Score)(cfg, sd, "cuda", dtype)
        a, b = _pixels(3, side, 7), _pixels(3, side, 8)
        b[1] = a[1] + 0.3 * b[1]                            # a near pair, an unrelated pair, an identical pair
        b[2] = a[2]
        for L in (0, 2):
            got = sc.score_pixel_pairs(a, b, L).double().cpu()
            want = R.score(sd, cfg, a, b, L)
            err = (got - want).abs()
            worst = max(worst, float(err.max()))
            if dtype == torch.float32:
                assert bool((err <= 1e-4 * want.abs()).all()), (kind, side, L, got, want)
            else:
                # measured maxima (MI355X): dinov2 bf16 1.0e-3, fp16 6.9e-5; clip bf16 1.8e-3, fp16 1.4e-4
                assert float(err.max()) <= 3e-2, (kind, side, L, got, want)
            assert abs(float(got[2]) - 1.0) <= 1e-6, got                      # score(A, A) = 1: no noise, no slot
            back = sc.score_pixel_pairs(b, a, L).double().cpu()
            assert float((back - got).abs().max()) <= 1e-6, (got, back)      # score(A, B) = score(B, A)
        m = sc.score_pixel_pairs(a, b, 1, "mse").double().cpu()
        wm = R.score(sd, cfg, a, b, 1, "mse")
        assert float(m[2]) == 0.0
        if dtype == torch.float32:
            assert bool(((m - wm).abs() <= 1e-4 * wm.abs()).all()), (m, wm)
        else:
            assert float((m - wm).abs().max()) <= 3e-2, (m, wm)
    print(f"vit pair scores {kind} {dtype}: max |score - float64| = {worst:.3e}")


# ---- 3. the projected tail directly ---------------------------------------------------------------------------------------------------
def _features(H, N, D, n_feat, dtype, seed=0):
    """q, k, v [n_feat][1][N][H*D] with logit std about 2 (q and k of std sqrt(2): q.k / sqrt(D) then has std 2), the images related
    (a shared base plus each image's own part) so that scores are neither 0 nor 1; W with unit row gain and a bias of 0.1."""
    g = torch.Generator().manual_seed(1000 * N + H + seed)
    Cc = H * D
    base = [torch.randn(1, 1, N, Cc, generator=g) for _ in range(3)]
    own = [torch.randn(n_feat, 1, N, Cc, generator=g) for _ in range(3)]
    q, k, v = ((0.8 * b + 0.6 * o) * s for b, o, s in zip(base, own, (2 ** 0.5, 2 ** 0.5, 1.0)))
    w = torch.randn(Cc, Cc, generator=g) / Cc ** 0.5
    bias = 0.1 * torch.randn(Cc, generator=g)
    return [t.to(dtype).cuda().contiguous() for t in (q, k, v, w)] + [bias.cuda()]


def _idx(pairs):
    ia = torch.tensor([p[0] for p in pairs], dtype=torch.int32).cuda()
    ib = torch.tensor([p[1] for p in pairs], dtype=torch.int32).cuda()
    return ia, ib


PAIRS5 = [(0, 1), (2, 1), (0, 0), (1, 0), (2, 3)]          # repeated images, an image against itself, a pair and its mirror


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("H,N,D", [(2, 26, 64), (2, 257, 64), (12, 50, 64)], ids=["2x26x64", "2x257x64", "12x50x64-B32"])
def test_pair_score_proj_against_float64(H, N, D, dtype):
    from diffsim_amd.engine import pair_score, pair_score_proj
    q, k, v, w, bias = _features(H, N, D, 4, dtype)
    worst = {}
    for sim in ("cosine", "mse"):
        ia, ib = _idx(PAIRS5)
        got, st = pair_score_proj(q, k, v, ia, ib, H, sim, return_status=True, w_out=w, bias=bias)
        want = R.pair_scores(q.cpu(), k.cpu(), v.cpu(), ia.tolist(), ib.tolist(), H, sim, w.cpu(), bias.cpu())
        err = (got.double().cpu() - want).abs()
        worst[sim] = float(err.max())
        assert not st.any()
        if dtype == torch.float32:
            assert bool((err <= 1e-4 * want.abs().clamp_min(1e-3)).all()), (sim, got, want)
        else:
            # measured maxima over the three shapes (MI355X): bf16 cosine 1.2e-4, mse 1.6e-4; fp16 cosine 1.3e-5,
            # mse 1.4e-5
            assert float(err.max()) <= 3e-2, (sim, got, want)
        assert abs(float(got[2]) - (1.0 if sim == "cosine" else 0.0)) <= 1e-6            # an image against itself
        assert float(got[0]) == float(got[3])                                             # a pair and its mirror: the same two directions
        # deterministic; batch-invariant: each pair alone is the pair in the batch, bit for bit (n_pairs 1)
        again = pair_score_proj(q, k, v, ia, ib, H, sim, w_out=w, bias=bias)
        assert torch.equal(again, got)
        for p in (0, 4):
            alone = pair_score_proj(q, k, v, ia[p:p + 1].contiguous(), ib[p:p + 1].contiguous(), H, sim, w_out=w, bias=bias)
            assert torch.equal(alone, got[p:p + 1]), (sim, p)
        # W = I, b = 0: the plain pair tail
        eye, zero = torch.eye(H * D, dtype=dtype).cuda(), torch.zeros(H * D).cuda()
        plain = pair_score(q, k, v, ia, ib, H, sim)
        ident = pair_score_proj(q, k, v, ia, ib, H, sim, w_out=eye, bias=zero)
        assert float((ident - plain).abs().max()) <= 1e-6 * max(1.0, float(plain.abs().max())), (ident, plain)
        # the bias is part of the score
        nobias = pair_score_proj(q, k, v, ia, ib, H, sim, w_out=w, bias=zero)
        if sim == "cosine":
            assert float((nobias - got).abs()[[0, 1, 4]].min()) > 1e-5
    print(f"pair_score_proj H{H} N{N} D{D} {dtype}: max |score - float64| cosine {worst['cosine']:.3e} mse {worst['mse']:.3e}")


def test_pair_score_proj_nan_features_raise_their_pairs_status_only():
    from diffsim_amd.engine import pair_score_proj
    H, N, D = 2, 26, 64
    q, k, v, w, bias = _features(H, N, D, 4, torch.bfloat16)
    ia, ib = _idx(PAIRS5)
    clean = pair_score_proj(q, k, v, ia, ib, H, w_out=w, bias=bias)
    v[3, 0, 5, 70] = float("nan")
    got, st = pair_score_proj(q, k, v, ia, ib, H, return_status=True, w_out=w, bias=bias)
    assert st.tolist() == [0, 0, 0, 0, 1] and not torch.isfinite(got[4])
    assert torch.equal(got[:4], clean[:4])


def test_pair_score_proj_refusals_enqueue_nothing():
    """DSIM_ERR_INVALID (-1): a head dim outside the list, a bad dtype, n_pairs < 1, 2 n_pairs > 65535; DSIM_ERR_WORKSPACE (-3): a
    short workspace; the workspace query is 0 for the former.  The outputs keep their sentinel."""
    L = _lib.lib()
    H, N, D = 2, 26, 64
    q, k, v, w, bias = _features(H, N, D, 2, torch.bfloat16)
    ia, ib = _idx([(0, 1)])
    out = torch.full((4,), -7.0, device="cuda")
    st = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    need = L.dsim_pair_score_proj_workspace_bytes(1, 1, H, N, D, _lib.DSIM_BF16)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(n_pairs=1, heads=H, D=D, dtype=_lib.DSIM_BF16, sim=0, ws_bytes=need, w_ptr=w.data_ptr()):
        return L.dsim_pair_score_proj(q.data_ptr(), k.data_ptr(), v.data_ptr(), ia.data_ptr(), ib.data_ptr(), n_pairs, 1, heads, N, D, dtype,
                                      sim, w_ptr, bias.data_ptr(), out.data_ptr(), st.data_ptr(), ws.data_ptr(), ws_bytes, None)
    Q = L.dsim_pair_score_proj_workspace_bytes
    assert call(D=48, heads=1) == -1 and Q(1, 1, 1, N, 48, _lib.DSIM_BF16) == 0
    assert call(dtype=7) == -1 and Q(1, 1, H, N, D, 7) == 0
    assert call(n_pairs=0) == -1 and Q(0, 1, H, N, D, _lib.DSIM_BF16) == 0
    assert call(n_pairs=32768) == -1 and Q(32768, 1, H, N, D, _lib.DSIM_BF16) == 0
    assert Q(32767, 1, H, N, D, _lib.DSIM_BF16) > 0
    assert call(sim=2) == -1
    assert call(w_ptr=None) == -1
    assert call(ws_bytes=need - 257) == -3
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((st == -7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert float(out[0]) != -7.0 and int(st[0]) == 0 and bool((out[1:] == -7.0).all())


# ---- 4. files in: the reference's entry points, triplets, the retrieval matrix ------------------------------------------------------
def _scorer(kind, dtype, weights):
    from diffsim_amd.vit import CLIPScore, Dinov2Score, Preprocess, CLIP_MEAN, CLIP_STD, IMAGENET_MEAN, IMAGENET_STD
    pre = Preprocess(48, 40, *((CLIP_MEAN, CLIP_STD) if kind == "clip" else (IMAGENET_MEAN, IMAGENET_STD)))
    return (CLIPScore if kind == "clip" else Dinov2Score)(_cfg(kind, 40), weights[(kind, 40)], "cuda", dtype, pre), pre


@pytest.mark.parametrize("kind", ["clip", "dinov2"])
def test_files_in_equals_pixels_in(kind, weights):
    from PIL import Image
    from diffsim_amd import harness as H, retrieval as Rt
    sc, pre = _scorer(kind, torch.float32, weights)
    cross = sc.clip_cross_score if kind == "clip" else sc.dino_cross_score
    a, b, c, d = IMGS
    px = {p: pre(Image.open(p)) for p in IMGS}
    s = cross(a, b, [2])
    assert s.shape == (1,) and torch.equal(s, sc.score_pixel_pairs(px[a], px[b], 2))
    assert torch.equal(cross(Image.open(a), [Image.open(b)], [2]), s)                        # PIL images, lists
    want = R.score(weights[(kind, 40)], sc.cfg, px[a], px[b], 2)
    assert abs(float(s) - float(want)) <= 1e-4 * abs(float(want))
    both = cross([a, c], [b, d], [1])
    assert both.shape == (2,) and torch.equal(both[1:], cross(c, d, [1]))
    with pytest.raises(ValueError):
        cross(a, b, [1, 2])
    # triplets: 3 forwards per triplet, one tail launch per chunk -- the pairwise calls bit for bit
    trip = [(a, b, c, "p"), (d, c, a, "q"), (b, a, d, "p")]
    sl, sr, bad = H.score_path_triplets(sc, trip, 512, "up_blocks", [1], 600, 2333, "cosine", batch_triplets=2, unet_triplets=2)
    assert bad == 0
    for i, t in enumerate(trip):
        assert torch.equal(sl[i], cross(t[0], t[1], [1])[0]) and torch.equal(sr[i], cross(t[0], t[2], [1])[0]), i
    # tap sweep from files: each row the one-tap scores
    rows = sc.score_pairs_taps([(a, b), (c, d)], [2, 0])
    assert rows.shape == (2, 2)
    for r, L in enumerate((2, 0)):
        assert torch.equal(rows[r], cross([a, c], [b, d], [L])), L
    if kind == "clip":
        with pytest.raises(_lib.DsimError, match="no score matrix"):
            Rt.score_path_matrix(sc, [a, b], [c, d], 512, None, "up_blocks", [1])
        return
    # retrieval: the plain score matrix serves dino_cross; cells against pair scores within tests/test_gpu_matrix.py's bounds
    for dtype in DTYPES:
        sd_, _ = _scorer(kind, dtype, weights)
        m = Rt.score_path_matrix(sd_, [a, b, c], [b, c, d, a], 512, None, "up_blocks", [1], 600, 2333, "cosine").cpu()
        p = sd_.dino_cross_score([a] * 4 + [b] * 4 + [c] * 4, [b, c, d, a] * 3, [1]).view(3, 4).cpu()
        if dtype == torch.float32:
            assert ((m - p).abs() / p.abs().clamp_min(1e-6)).max().item() <= 1e-5, (m, p)
        else:
            assert ((m - p).abs() / p.abs().clamp_min(1e-3)).max().item() <= 4e-3, (m, p)


# ---- 5. the command line, end to end --------------------------------------------------------------------------------------------------
def _run_cli(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "diffsim_amd"] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


def _cute_tree(root):
    from PIL import Image
    n = 0
    for cls in ("mug", "shoe"):
        for inst in ("inst0", "inst1"):
            folder = os.path.join(root, cls, inst, "light0")
            os.makedirs(folder)
            for j in range(2):
                Image.open(IMGS[n % 4]).rotate(90 * (n // 4)).save(os.path.join(folder, f"im{j}.png"))
                n += 1


@pytest.mark.parametrize("metric", ["clip_cross", "dino_cross"])
def test_cli_end_to_end(metric, tmp_path):
    from tests.test_vit_host import _write_checkpoint
    kind = "clip" if metric == "clip_cross" else "dinov2"
    ckpt = str(tmp_path / "ckpt")
    _write_checkpoint(ckpt, _cfg(kind, 40), "vision_model." if kind == "clip" else "")
    tree = str(tmp_path / "cute")
    _cute_tree(tree)
    r = _run_cli(["--metric", metric, "--dataset", "cute", "--model_path", ckpt, "--image_path", tree, "--target_layer", "1",
                  "--similarity", "cosine", "--dtype", "fp32", "--decode_procs", "0"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "--image_size is not consulted" in r.stdout and "Total comparisons: 40" in r.stdout and "Accuracy:" in r.stdout, r.stdout
    out = str(tmp_path / "rank")
    args = ["--metric", metric, "--dataset", "retrieval", "--model_path", ckpt, "--query_path", os.path.join(tree, "mug"), "--image_path",
            os.path.join(tree, "shoe"), "--out_path", out, "--target_layer", "1", "--similarity", "cosine", "--dtype", "bf16", "--topk", "3"]
    r = _run_cli(args)
    if metric == "clip_cross":
        assert r.returncode == 2 and "no projected score matrix" in r.stderr, r.stdout + r.stderr
        return
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Score matrix (4, 4)" in r.stdout, r.stdout
    files = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert len(files) == 4 and all(f.endswith(".txt") for f in files), files
