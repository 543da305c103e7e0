"""diffeats / dinofeats on the GPU: the feature kernels (csrc/feats.hip: attention outputs, projection, min-max normalisation,
stats), the pair cosine, the Gram matrix, and the scorers and command line on top (diffsim_amd/feats.py), against the float64
restatement tests/_feats64.py, which tests/test_feats_host.py pins to plain torch.

Bounds.  On a cosine, against float64 fed the same rounded inputs, the project's own for this attention arithmetic
(tests/test_gpu_matrix.py): 4e-3 absolute in bf16, 5e-4 in fp16, 1e-5 relative in f32.  The projection and the normalisation add two
rounding steps, so wherever features are built from q, k, v the test also measures, on the CPU, a plain torch restatement IN the
compute dtype (tests/_feats64.py restate) against float64 on the same inputs; if that error exceeds half of the bound, the bound of
the case is twice the measured error -- never a figure taken from the kernel.  A feature element gets one ulp of the compute dtype
at its magnitude plus that bound times max |F|.  Every test prints its figures before it asserts.
Measured on the CPU, the restatement's element error over max |F| (and the bound that follows): context layer 6 x 64 heads, 50
tokens: bf16 4.1e-3 (8.3e-3), fp16 5.2e-4 (1.0e-3), f32 3.2e-7 (stays 1e-5); C = 320 projection + min-max: 7.8e-3 (1.6e-2), 9.8e-4
(2.0e-3), 1.8e-7; C = 1280, 130 tokens: 1.2e-2 (2.3e-2), 9.8e-4 (2.0e-3), 1.9e-7; one token: 0.  The restatement's error on the
cosine stays under 7e-5 everywhere, so every score keeps the project's bound.  Measured on an MI355X, the kernels' own errors: elements
4.1e-3 / 5.2e-4 / 4.2e-7 of max |F| (bf16 / fp16 / f32: one ulp at the maximum), pair scores from q, k, v 2.0e-5 / 1.6e-6 / 6.4e-8,
pair scores and matrix cells of given features 3.0e-7 (f32: 1.5e-6 relative), a cell against its pair score 3.0e-7 (f32 9.5e-7),
files in 1.8e-4 / 2.3e-5 / 6.7e-8, score(A, A) - 1 at most 8.3e-7.
"""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from diffsim_amd import _lib, config as C, synth as S
from tests import _feats64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
IMGS = [os.path.join(GOLDEN, f"g1_img_{c}.png") for c in "abcd"]
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
IDS = ["bf16", "fp16", "fp32"]
BOUND = {torch.bfloat16: 4e-3, torch.float16: 5e-4, torch.float32: 1e-5}
MANT = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


def ulp(x, dtype):
    """one unit in the last place of `dtype` at the magnitude of each element of the float64 tensor x"""
    bits, emin = MANT[dtype]
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, e - bits)


def effective(bound, measured):
    """the issue's rule: the project's bound, or twice the restatement's measured error where that exceeds half of it"""
    return bound if measured <= 0.5 * bound else 2.0 * measured


def cos_close(got, want, dtype, bound=None):
    """|got - want| within the bound: absolute in the 16-bit modes, relative in f32"""
    bound = BOUND[dtype] if bound is None else bound
    err = (got.double().cpu() - want).abs()
    if dtype == torch.float32:
        err = err / want.abs().clamp_min(1e-6)
    return float(err.max()), bound


def _qkv(n, B, H, N, D, dtype, seed, correlate=0.5):
    g = torch.Generator().manual_seed(seed)
    base = [torch.randn(1, B, N, H * D, generator=g) for _ in range(3)]
    return tuple((correlate * b + (1 - correlate) * torch.randn(n, B, N, H * D, generator=g)).to(dtype).cuda().contiguous() for b in base)


def _proj(Cc, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.randn(Cc, Cc, generator=g) / math.sqrt(Cc)).to(dtype).cuda().contiguous(),
            (0.2 * torch.randn(Cc, generator=g)).cuda().contiguous())


# ---- 1. features from q, k, v, element by element -----------------------------------------------------------------------------------
SHAPES = [((3, 2, 2, 1, 40), False), ((2, 1, 6, 50, 64), False), ((2, 2, 8, 64, 40), True), ((2, 2, 8, 130, 160), True)]
_REF = {}


def _reference(shape, proj, dtype):
    """the case's inputs, float64 features and restatement error, computed once and shared"""
    key = (shape, proj, dtype)
    if key not in _REF:
        n, B, H, N, D = shape
        q, k, v = _qkv(n, B, H, N, D, dtype, 100 + N)
        w, b = _proj(H * D, dtype, 7) if proj else (None, None)
        want, wstats = R.features64(q, k, v, H, dtype, w, b, proj)
        rest = R.restate(q, k, v, H, w, b, proj).double()
        scale = float(want.abs().max())
        _REF[key] = dict(q=q, k=k, v=v, w=w, b=b, want=want, wstats=wstats, scale=scale,
                         rest_elem=float((rest - want).abs().max()) / scale,
                         rest_cos=abs(R.cosine64(rest[0], rest[1]) - R.cosine64(want[0], want[1])))
    return _REF[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,proj", SHAPES, ids=["one-token", "dino-small", "C320-proj-minmax", "C1280-proj-minmax"])
def test_features_against_float64(eng, shape, proj, dtype):
    """(n, B, H, N, D): one token; DINOv2-small's heads with an odd token count; C = 320 and C = 1280 (across the 128-query tile)
    with the projection and the min-max normalisation."""
    n, B, H, N, D = shape
    r = _reference(shape, proj, dtype)
    feats, stats = eng.attn_features(r["q"], r["k"], r["v"], H, r["w"], r["b"], minmax=proj)
    assert feats.shape == r["q"].shape and feats.dtype == dtype and stats.shape == (n, 4) and stats.dtype == torch.float32
    got, want = feats.double().cpu(), r["want"]
    bound = effective(BOUND[dtype], r["rest_elem"])
    err = (got - want).abs()
    tol = ulp(want, dtype) + bound * r["scale"]
    print(f"features {shape} {dtype}: max err {float(err.max()):.3e}, max |F| {r['scale']:.3e}, restatement {r['rest_elem']:.3e} of max |F|, "
          f"bound {bound:.3e}")
    assert bool((err <= tol).all()), float((err - tol).max())
    # stats: the sum of squares against float64 on the rounded features the call wrote (a chain of 64 f32 fmas per thread and a
    # 10-step tree of positive terms: (64 + 10 + 2) 2^-24 relative), min and max exactly
    st = stats.double().cpu()
    ss = (got * got).sum((1, 2, 3))
    print(f"  sum of squares: relative error {float(((st[:, 0] - ss).abs() / ss).max()):.3e}")
    assert bool(((st[:, 0] - ss).abs() <= 76 * 2.0 ** -24 * ss).all())
    assert bool((st[:, 3] == 0).all())
    if not proj:
        assert torch.equal(st[:, 1], got.amin((1, 2, 3))) and torch.equal(st[:, 2], got.amax((1, 2, 3)))
    else:                       # (mn, mx) are F's: against float64 within an element's bound; G spans [0, 1] exactly
        fscale = r["wstats"][:, 1:].abs().max()
        assert bool(((st[:, 1:3] - r["wstats"][:, 1:]).abs() <= ulp(r["wstats"][:, 1:], dtype) + bound * fscale).all())
        assert bool((got.amin((1, 2, 3)) == 0).all()) and bool((got.amax((1, 2, 3)) == 1).all())
    # the pair score of the first two images against float64, from the same q, k, v
    ia, ib = torch.tensor([0], dtype=torch.int32).cuda(), torch.tensor([1], dtype=torch.int32).cuda()
    s, status = eng.feature_pair_score(feats, stats, ia, ib, return_status=True)
    e, cb = cos_close(s, torch.tensor([R.cosine64(want[0], want[1])], dtype=torch.float64), dtype, effective(BOUND[dtype], r["rest_cos"]))
    print(f"  pair score: err {e:.3e}, restatement {r['rest_cos']:.3e}, bound {cb:.3e}")
    assert e <= cb and int(status[0]) == 0
    # an image's features and stats do not depend on the other images of the call
    f1, s1 = eng.attn_features(r["q"][1:2].contiguous(), r["k"][1:2].contiguous(), r["v"][1:2].contiguous(), H, r["w"], r["b"], minmax=proj)
    assert torch.equal(f1[0], feats[1]) and torch.equal(s1[0], stats[1])


def test_feature_call_refusals(eng):
    q, k, v = _qkv(2, 1, 2, 5, 16, torch.bfloat16, 3)
    w, b = _proj(32, torch.bfloat16, 4)
    with pytest.raises(_lib.DsimError):
        eng.attn_features(q, k, v, 2, w_out=w)                          # a weight without its bias
    with pytest.raises(_lib.DsimError):
        eng.attn_features(q, k, v, 2, w.float(), b)                     # another dtype
    L = _lib.lib()
    need = L.dsim_attn_features_workspace_bytes(2, 1, 2, 5, 16, 160, _lib.DSIM_BF16, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    feats, stats = torch.full_like(q, -7.0), torch.full((2, 4), -7.0, device="cuda")
    call = lambda L_=160, wsb=need: L.dsim_attn_features(q.data_ptr(), k.data_ptr(), v.data_ptr(), 2, 1, 2, 5, 16, L_, _lib.DSIM_BF16, None,
                                                          None, 0, feats.data_ptr(), stats.data_ptr(), ws.data_ptr(), wsb, None)
    assert call(L_=168) == -1 and call(wsb=need - 257) == -3
    torch.cuda.synchronize()
    assert bool((feats == -7.0).all()) and bool((stats == -7.0).all())      # every check before anything is enqueued
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((stats[:, 3] == 0).all())


# ---- 2. pair scores and matrices of given features ------------------------------------------------------------------------------------
def _set(n, L, dtype, seed, base_seed=1):
    """n feature vectors that resemble a common base by different amounts: cosines spread between about 0.2 and 0.8"""
    base = torch.randn(L, generator=torch.Generator().manual_seed(base_seed))
    c = torch.linspace(0.35, 0.65, n)[:, None]
    x = (c * base + (1 - c) * torch.randn(n, L, generator=torch.Generator().manual_seed(seed))).to(dtype)
    stats = torch.zeros(n, 4)
    stats[:, 0] = (x.double() ** 2).sum(1).float()
    return x.cuda().contiguous(), stats.cuda()


def _all_pairs(eng, fa, fb):
    na, nb = fa[0].shape[0], fb[0].shape[0]
    x, st = torch.cat([fa[0], fb[0]]).contiguous(), torch.cat([fa[1], fb[1]]).contiguous()
    ia = torch.arange(na, dtype=torch.int32).repeat_interleave(nb).cuda()
    ib = (na + torch.arange(nb, dtype=torch.int32)).repeat(na).cuda()
    return eng.feature_pair_score(x, st, ia, ib).view(na, nb)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("na,nb,L", [(3, 5, 560), (33, 34, 560), (2, 3, 332800)], ids=["edge-tiles", "across-a-tile", "split-K"])
def test_pairs_and_matrix_against_float64(eng, na, nb, L, dtype):
    """3 x 5: edge tiles only; 33 x 34 at L = 560 (B = 1, N = 7, C = 80): across a 32-row tile, L no multiple of a K stage; 2 x 3 at
    L = 332 800: 21 split-K partials per cell.  Both paths hold the bound; they are close to each other, not bit-equal."""
    fa, fb = _set(na, L, dtype, 11), _set(nb, L, dtype, 12)
    want = R.matrix64(fa[0], fb[0])
    tol = BOUND[dtype]
    spread = float(want.max() - want.min())
    assert spread >= 10 * tol, spread                          # the comparison has teeth
    m, st = eng.feature_matrix(fa, fb, return_status=True)
    p = _all_pairs(eng, fa, fb)
    em, _ = cos_close(m, want, dtype)
    ep, _ = cos_close(p, want, dtype)
    print(f"{na} x {nb}, L {L}, {dtype}: matrix err {em:.3e}, pair err {ep:.3e}, bound {tol:.1e}, spread {spread:.3f}, "
          f"matrix vs pair {float((m - p).abs().max()):.3e}")
    assert m.shape == (na, nb) and m.dtype == torch.float32 and not bool(st.any())
    assert em <= tol and ep <= tol
    assert torch.equal(m, eng.feature_matrix(fa, fb)) and torch.equal(p, _all_pairs(eng, fa, fb))       # deterministic


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cell_independence(eng, dtype):
    """A cell depends on its two images alone: the 33 x 34 matrix's cells as 1 x 1 calls, a 5 x 3 sub-block and the transposed call;
    a pair alone and inside a batch of 7."""
    fa, fb = _set(33, 560, dtype, 21), _set(34, 560, dtype, 22)
    m = eng.feature_matrix(fa, fb)
    sub = lambda f, sl: (f[0][sl].contiguous(), f[1][sl].contiguous())
    for i, j in ((0, 0), (32, 33), (31, 5), (7, 32)):
        assert torch.equal(eng.feature_matrix(sub(fa, slice(i, i + 1)), sub(fb, slice(j, j + 1)))[0, 0], m[i, j]), (i, j)
    assert torch.equal(eng.feature_matrix(sub(fa, slice(28, 33)), sub(fb, slice(31, 34))), m[28:33, 31:34])
    assert torch.equal(eng.feature_matrix(fb, fa).T, m)
    ia = torch.tensor([3, 0, 32, 5, 5, 17, 9], dtype=torch.int32).cuda()
    ib = torch.tensor([4, 1, 31, 5, 6, 2, 30], dtype=torch.int32).cuda()
    batch = eng.feature_pair_score(*fa, ia, ib)
    for t in range(7):
        assert torch.equal(eng.feature_pair_score(*fa, ia[t:t + 1].contiguous(), ib[t:t + 1].contiguous())[0], batch[t]), t
    # score(A, A): the dot and the norms fold separately, so within 1e-6 of 1, not exactly 1
    self_m = eng.feature_matrix(fa, fa).diagonal()
    idx = torch.arange(33, dtype=torch.int32).cuda()
    self_p = eng.feature_pair_score(*fa, idx, idx)
    print(f"self scores {dtype}: matrix {float((self_m - 1).abs().max()):.3e}, pair {float((self_p - 1).abs().max()):.3e}")
    assert float((self_m - 1).abs().max()) <= 1e-6 and float((self_p - 1).abs().max()) <= 1e-6


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_degenerate_normalisation_poisons_its_own_image_only(eng, dtype):
    """w_out = 0 with a constant bias makes one image's F constant: mx == mn, every value NaN, as the reference's division gives.
    Its pairs and its matrix row (or column) are NaN with status 1; every other cell is bit for bit the call without it."""
    n, B, H, N, D = 4, 2, 2, 20, 40
    q, k, v = _qkv(n, B, H, N, D, dtype, 31)
    w, b = _proj(H * D, dtype, 32)
    feats, stats = eng.attn_features(q, k, v, H, w, b, minmax=True)
    one = lambda t: t[2:3].contiguous()
    fz, sz = eng.attn_features(one(q), one(k), one(v), H, torch.zeros_like(w), torch.full_like(b, 0.25), minmax=True)
    assert bool(torch.isnan(fz.float()).all()) and bool(torch.isnan(sz[0, 0])) and float(sz[0, 1]) == float(sz[0, 2]) == 0.25
    feats, stats = feats.clone(), stats.clone()
    feats[2], stats[2] = fz[0], sz[0]
    gq, gk, gv = _qkv(5, B, H, N, D, dtype, 33)
    gal = eng.attn_features(gq, gk, gv, H, w, b, minmax=True)
    keep = [0, 1, 3]
    m, st = eng.feature_matrix((feats, stats), gal, return_status=True)
    clean = eng.feature_matrix((feats[keep].contiguous(), stats[keep].contiguous()), gal)
    assert bool(torch.isnan(m[2]).all()) and bool((st[2] == 1).all()) and not bool(st[keep].any())
    assert torch.equal(m[keep], clean)
    mt, stt = eng.feature_matrix(gal, (feats, stats), return_status=True)
    assert bool(torch.isnan(mt[:, 2]).all()) and bool((stt[:, 2] == 1).all()) and torch.equal(mt[:, keep], clean.T)
    ia = torch.tensor([0, 2, 1, 3], dtype=torch.int32).cuda()
    ib = torch.tensor([1, 3, 2, 0], dtype=torch.int32).cuda()
    s, ps = eng.feature_pair_score(feats, stats, ia, ib, return_status=True)
    assert ps.tolist() == [0, 1, 1, 0] and bool(torch.isnan(s[1:3]).all())
    alone = eng.feature_pair_score(feats, stats, ia[[0, 3]].contiguous(), ib[[0, 3]].contiguous())
    assert torch.equal(s[[0, 3]], alone)


# ---- 3. end to end: files in, the scorers, triplets, retrieval, the command line ----------------------------------------------------
def _dino(dtype):
    from diffsim_amd.vit import Dinov2Score, Preprocess, IMAGENET_MEAN, IMAGENET_STD
    pre = Preprocess(48, 40, IMAGENET_MEAN, IMAGENET_STD)
    return Dinov2Score(C.VIT_TINY_DINO, S.make_state_dict(C.VIT_TINY_DINO, 3), "cuda", dtype, pre), pre


def _sd15(dtype):
    from diffsim_amd.diffsim import DiffSim
    from tests._fakes import FakeVAE
    ctx = S.make_context(C.TINY)
    return DiffSim(torch_dtype=dtype, device="cuda", unet_config=C.TINY, state_dict=S.make_state_dict(C.TINY, seed=0), vae=FakeVAE(),
                   encode_prompt=lambda p: ctx)


def _views(dtype):
    """(metric, view, pairwise score of two files [at a tap], two taps of a sweep, (q, k, v, heads, attn_features keywords) of two
    files) for both metrics"""
    from PIL import Image
    from diffsim_amd import feats as Fm
    from diffsim_amd.inputs import path_latents
    from diffsim_amd.scorer import stack_rows
    dino, pre = _dino(dtype)
    dview = Fm.FeatureView(dino)
    yield ("dinofeats", dview, lambda x, y, tap=1: dino.dino_feature_score(x, y, [tap]), [1, 0],
           lambda x, y: (*dino.features(torch.cat([pre(Image.open(x)), pre(Image.open(y))]), 1), dino.cfg.num_heads, dview.spec(1)))
    ds = _sd15(dtype)
    view = Fm.FeatureView(ds)

    def operands(x, y):
        (la, lb), nA, nB = path_latents(ds, [(x, y)], (0, 1), 128, 2334, 1)
        q, k, v = ds.features(*stack_rows([la, lb], [nA, nB], 0, 1), "p", "up_blocks", 1, 600)
        return q, k, v, ds.engine("up_blocks", 1).heads, view.spec(("up_blocks", 1))
    yield ("diffeats", view, lambda x, y, tap=("up_blocks", 1): Fm.diffeats(x, y, 128, ds, "p", tap[0], [tap[1]], 600, seed=2334),
           [("up_blocks", 1), ("down_blocks", 0)], operands)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_files_in_against_float64_triplets_and_retrieval(dtype):
    from diffsim_amd import harness as H, retrieval as Rt, sweep
    a, b, c, d = IMGS
    for metric, view, pair, taps, operands in _views(dtype):
        s = pair(a, b)
        assert s.shape == (1,) and s.dtype == torch.float32, metric
        q, k, v, heads, spec = operands(a, b)
        want, _ = R.features64(q, k, v, heads, dtype, spec.get("w_out"), spec.get("bias"), spec["minmax"])
        rest = R.restate(q, k, v, heads, spec.get("w_out"), spec.get("bias"), spec["minmax"]).double()
        w64 = R.cosine64(want[0], want[1])
        bound = effective(BOUND[dtype], abs(R.cosine64(rest[0], rest[1]) - w64))
        e, _ = cos_close(s, torch.tensor([w64], dtype=torch.float64), dtype, bound)
        print(f"{metric} {dtype}: score {float(s):.6f}, float64 {w64:.6f}, err {e:.3e}, bound {bound:.3e}")
        assert e <= bound, metric
        # triplets: the reference image's features once per triplet, the pairwise calls bit for bit
        trip = [(a, b, c, "p"), (d, c, a, "p"), (b, a, d, "p")]
        sl, sr, bad = H.score_path_triplets(view, trip, 128, "up_blocks", [1], 600, 2334, "cosine", batch_triplets=2, unet_triplets=2)
        assert bad == 0
        for i, t in enumerate(trip):
            assert torch.equal(sl[i], pair(t[0], t[1])[0]) and torch.equal(sr[i], pair(t[0], t[2])[0]), (metric, i)
        # a tap sweep from files: each row the one-tap scores bit for bit
        rows = sweep.score_path_pairs_taps(view, [(a, b), (c, d)], 128, "p", taps, 600, "cosine", 2334)
        assert rows.shape == (2, 2), metric
        for r, tap in enumerate(taps):
            assert torch.equal(rows[r], torch.cat([pair(a, b, tap), pair(c, d, tap)])), (metric, tap)
        # retrieval: the Gram matrix within the bound of the pairwise scores (close, not bit-equal)
        m, nbad = Rt.score_path_matrix(view, [a, b, c], [b, c, d, a], 128, "p", "up_blocks", [1], 600, 2334, "cosine", batch=3,
                                       return_status=True)
        p = torch.stack([pair(x, y)[0] for x in (a, b, c) for y in (b, c, d, a)]).view(3, 4)
        e, _ = cos_close(m, p.double().cpu(), dtype)
        print(f"  3 x 4 matrix against the pairwise scores: {e:.3e}")
        assert m.shape == (3, 4) and nbad == 0 and e <= BOUND[dtype], metric


def test_clip_cross_still_has_no_score_matrix():
    from diffsim_amd import retrieval as Rt
    from diffsim_amd.vit import CLIPScore, Preprocess, CLIP_MEAN, CLIP_STD
    sc = CLIPScore(C.VIT_TINY_CLIP, S.make_state_dict(C.VIT_TINY_CLIP, 3), "cuda", torch.float32, Preprocess(48, 40, CLIP_MEAN, CLIP_STD))
    with pytest.raises(_lib.DsimError, match="no score matrix"):
        Rt.score_path_matrix(sc, IMGS[:2], IMGS[2:], 512, None, "up_blocks", [1])


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


def test_cli_dinofeats_cute_then_retrieval(tmp_path, capsys):
    from diffsim_amd import cli
    from tests.test_vit_host import _write_checkpoint
    ckpt, tree, out = str(tmp_path / "ckpt"), str(tmp_path / "cute"), str(tmp_path / "rank")
    _write_checkpoint(ckpt, C.VIT_TINY_DINO)
    _cute_tree(tree)
    base = ["--metric", "dinofeats", "--model_path", ckpt, "--target_layer", "1", "--similarity", "cosine", "--decode_procs", "0"]
    assert cli.main(base + ["--dataset", "cute", "--image_path", tree, "--dtype", "fp32"]) == 0
    text = capsys.readouterr().out
    assert "--image_size is not consulted" in text and "Total comparisons: 40" in text and "Accuracy:" in text, text
    assert cli.main(base + ["--dataset", "retrieval", "--query_path", os.path.join(tree, "mug"), "--image_path", os.path.join(tree, "shoe"),
                            "--out_path", out, "--dtype", "bf16", "--topk", "3"]) == 0
    assert "Score matrix (4, 4)" in capsys.readouterr().out
    files = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert len(files) == 4 and all(f.endswith(".txt") for f in files), files


def test_cli_diffeats_cute(tmp_path, capsys, monkeypatch):
    from diffsim_amd import cli, loader
    from tests.test_cli import _write_checkpoint
    ckpt, tree = str(tmp_path / "ckpt"), str(tmp_path / "cute")
    os.makedirs(ckpt)
    _write_checkpoint(ckpt)
    _cute_tree(tree)
    monkeypatch.setattr(loader.LazyTokenizer, "__call__",
                        lambda self, p: torch.tensor([[0] + [3 + (ord(c) % 900) for c in p][:75] + [999] * (76 - min(75, len(p)))]))
    assert cli.main(["--metric", "diffeats", "--dataset", "cute", "--model_path", ckpt, "--image_path", tree, "--image_size", "128",
                     "--target_layer", "1", "--similarity", "cosine", "--dtype", "fp32", "--batch", "2", "--decode_procs", "0"]) == 0
    text = capsys.readouterr().out
    assert "taken literally" in text and "Experiment on up_blocks, layer [1]" in text and "Total comparisons: 40" in text, text
    assert "WARNING" not in text, text
