"""Soft region scores (dsim_pair_score_weights / engine.pair_score_weights): the region score with a byte weight per token.
Checked to the bit against engine.pair_score_regions where every byte is 0 or 255, against the float64 restatement
tests/_soft64.py for general weights, and for what the header promises: weights are multiplicities, a pair depends on its two images
and their weights alone, rows of weight 0 are never read, an image without weight is reported.

Features and tolerances are test_gpu_regions.py's _feats and _score_tol / _score_err / _gate, restated here."""
import ctypes

import pytest
import torch

from tests._soft64 import Soft64, soft64
from tests._tail64 import heads64

pytestmark = pytest.mark.gpu

B = 2
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SIZES = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 255]
SIMS = ("cosine", "mse")


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


def _feats(n, seed, dtype, N, H, D, logit_scale=1.0, correlate=0.5, channel_mean=0.0, cuda=True):
    """test_gpu_regions.py's features: per image noise plus a part shared by the images token by token; channel_mean: plus a part of
    v shared by every token of every image, as the channel means of real features are"""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(n, B, N, H * D, generator=g) for _ in range(3))
    base = tuple(torch.randn(1, B, N, H * D, generator=g) for _ in range(3))
    q, k, v = (correlate * b + (1 - correlate) * t for b, t in zip(base, (q, k, v)))
    q = q * logit_scale
    if channel_mean:
        v = v + channel_mean * torch.randn(1, B, 1, H * D, generator=g)
    ts = tuple(t.to(dtype).contiguous() for t in (q, k, v))
    return tuple(t.cuda() for t in ts) if cuda else ts


def _idx(*xs):
    return torch.tensor(list(xs), dtype=torch.int32).cuda()


def _positions(N, sizes, seed):
    """image i's sizes[i] listed tokens, at seeded positions, ascending"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(N, generator=g)[:r].sort().values for r in sizes]


def _weights(N, sizes, seed, lo=1, hi=255):
    """(len(sizes), N) uint8 on the GPU: image i has sizes[i] tokens at seeded positions with bytes uniform in lo .. hi, 0 elsewhere"""
    g = torch.Generator().manual_seed(seed + 1000)
    w = torch.zeros(len(sizes), N, dtype=torch.uint8)
    for i, pos in enumerate(_positions(N, sizes, seed)):
        w[i, pos] = torch.randint(lo, hi + 1, (len(pos),), generator=g).to(torch.uint8)
    return w.cuda()


def _poison(ts, w):
    """copies of q, k, v with NaN in every row of weight 0"""
    out = tuple(t.clone() for t in ts)
    for t in out:
        t.transpose(1, 2)[w == 0] = float("nan")              # (n, N, B, HD) view: every off row of every CFG half
    return out


def _score_tol(dtype, peaked):
    if dtype == torch.float32:
        return 1e-5
    if peaked:
        return 1e-2 if dtype == torch.bfloat16 else 2e-3
    return 4e-3 if dtype == torch.bfloat16 else 5e-4


def _score_err(got, want, sim, dtype):
    """cosine: absolute (relative in fp32); mse: relative"""
    if sim == "cosine" and dtype != torch.float32:
        return abs(got - want)
    return abs(got - want) / max(abs(want), 1e-6)


def _gate(dtype, peaked, sim):
    return _score_tol(dtype, peaked) * (1 if sim == "cosine" else 10)


# ---- 1. 0/255 weights are the region score, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("r", SIZES)
@pytest.mark.parametrize("D", [160, 40, 72, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_binary_weights_are_the_region_score_to_the_bit(eng, dtype, D, r):
    """Two images with r tokens of byte 255 at different positions inside N = 256 and byte 0 elsewhere: score and status of
    pair_score_regions on the mask m != 0.  The rows of weight 0 hold NaN: they are never read."""
    N, H = 256, 2
    ts = _feats(2, 100 + r + D, dtype, N, H, D)
    w = _weights(N, [r, r], 7 * r + D, 255, 255)
    assert not torch.equal(w[0], w[1]) and sorted(set(w.flatten().tolist())) == [0, 255]
    bad = _poison(ts, w)
    ia, ib = _idx(0, 1, 0), _idx(1, 0, 0)
    for sim in SIMS:
        want, wst = eng.pair_score_regions(*ts, w != 0, ia, ib, H, sim, return_status=True)
        got, st, sums = eng.pair_score_weights(*bad, w, ia, ib, H, sim, return_status=True, return_sums=True)
        assert torch.equal(got, want), (sim, got, want)
        assert torch.equal(st, wst) and st.tolist() == [0, 0, 0]
        assert sums.tolist() == [255 * r, 255 * r]


# ---- 2. general weights against float64 ------------------------------------------------------------------------------------------------
def _sizes(N):
    ok = [r for r in SIZES if r <= N]
    return [ok[-1], ok[len(ok) // 2], ok[1], ok[0]]


def _check64(eng, ts, w, pairs, H, dtype, peaked, label, scale=1):
    """every pair and both similarities against Soft64 (one set of float64 attentions for both); prints each error before it asserts
    and returns the largest error / gate ratio"""
    ref = Soft64(*ts, w, H, dtype)
    ia, ib = _idx(*(a for a, _ in pairs)), _idx(*(b for _, b in pairs))
    worst = 0.0
    for sim in SIMS:
        got, st = eng.pair_score_weights(*_poison(ts, w), w, ia, ib, H, sim, return_status=True)
        assert st.tolist() == [0] * len(pairs)
        want = [ref.pair(a, b, sim) for a, b in pairs]
        gate = scale * _gate(dtype, peaked, sim)
        errs = [_score_err(float(got[p]), want[p], sim, dtype) for p in range(len(pairs))]
        print(f"{label} {dtype} {sim} peaked={peaked}: errs {' '.join(f'{e:.3e}' for e in errs)} gate {gate:.1e}")
        for p, e in enumerate(errs):
            assert e <= gate, (sim, pairs[p], float(got[p]), want[p], e)
        worst = max(worst, max(errs) / gate)
    return worst


@pytest.mark.parametrize("N,H,D", [(256, 8, 160), (144, 2, 72), (200, 2, 160), (64, 4, 32), (256, 4, 40)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("peaked", [False, True])
def test_general_weights_match_float64(eng, dtype, N, H, D, peaked):
    """Four images with unequal numbers of listed tokens, bytes uniform in 1 .. 255; the pairs chain them and (1, 1) is an image with
    itself.  The values carry a channel mean, as in test_gpu_regions.py's float64 test and for its reason: the fp32 gate is relative,
    and a relative gate on a cosine measures the kernel only where the cosine is away from zero."""
    ts = _feats(4, 41 + N + D, dtype, N, H, D, logit_scale=4.0 if peaked else 1.0, channel_mean=1.0)
    w = _weights(N, _sizes(N), N + D)
    assert len(set(_sizes(N))) == 4
    _check64(eng, ts, w, [(0, 1), (1, 2), (2, 3), (3, 0), (1, 1)], H, dtype, peaked, f"N={N} H={H} D={D}")


@pytest.mark.parametrize("H,D", [(2, 160), (4, 40)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_light_key_with_the_largest_raw_logit(eng, dtype, H, D):
    """Every image has one key of byte 1 that most queries of every image like best before the bias: the queries share a component c
    per head and that key is a multiple of c.  The bias (-7.99 in log2 units) then changes the row maximum."""
    N = 256
    q, k, v = _feats(3, 17 + D, torch.float32, N, H, D, channel_mean=1.0, cuda=False)
    g = torch.Generator().manual_seed(D)
    c = torch.randn(H * D, generator=g)
    star = [5, 130, 255]
    q = q + 0.5 * c
    for i, u in enumerate(star):
        k[i, :, u] = (12.0 / D ** 0.5) * c                     # its logit: about 0.5 |c|^2 (12 / sqrt D) / sqrt D = 6
    ts = tuple(t.to(dtype).contiguous() for t in (q, k, v))
    w = _weights(N, [N, 200, 129], 3).cpu()
    for i, u in enumerate(star):
        w[i, u] = 1
    for i in range(3):                                          # the construction holds: raw argmax over the listed keys
        rows = torch.nonzero(w[i]).flatten()
        s = heads64(ts[0][(i + 1) % 3], H) @ heads64(ts[1][i], H).index_select(2, rows).transpose(-1, -2)
        assert (rows[s.argmax(-1)] == star[i]).double().mean() > 0.5
    _check64(eng, tuple(t.cuda() for t in ts), w.cuda(), [(0, 1), (1, 2), (2, 0), (1, 1)], H, dtype, False, f"light key D={D}")


@pytest.mark.parametrize("H,D", [(2, 160), (4, 40), (2, 64)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_heavy_keys_come_last(eng, dtype, H, D):
    """All N = 256 tokens are listed; the first 192 carry byte 1 and the last 64, the last key tile, bytes of 200 .. 255: the running
    maximum grows by about 8 (log2) in the last tile, so the accumulated outputs are re-based there."""
    N = 256
    ts = _feats(3, 23 + D, dtype, N, H, D, channel_mean=1.0)
    w = _weights(N, [N, N, N], 4, 200, 255)
    w[:, :192] = 1
    _check64(eng, ts, w, [(0, 1), (1, 2), (2, 2)], H, dtype, False, f"heavy last D={D}")


# ---- 3. weights are multiplicities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,D", [(2, 160), (4, 40)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_weight_is_a_multiplicity(eng, dtype, H, D):
    """X: 128 tokens with even bytes 2c.  X': 256 tokens, every token of X twice (identical q, k, v rows) with byte c each.  Y is the
    same image in both calls (its 128 tokens, then 128 rows of NaN with byte 0).  (X, Y) and (X', Y), and the mirrored pairs, agree
    within twice the float64 bound: each side carries its own rounding.  No oracle: the bias missing from either attention, or the
    query weight from any sum, breaks it."""
    n1 = 128
    ts = _feats(2, 57 + D, dtype, n1, H, D)
    g = torch.Generator().manual_seed(5)
    cx = torch.randint(1, 128, (n1,), generator=g)
    cx[::9] = 0                                                 # (some tokens of X have no weight at all)
    wy = torch.randint(0, 256, (n1,), generator=g)
    small_w = torch.stack([2 * cx, wy]).to(torch.uint8).cuda()
    twice = tuple(torch.stack([t[0].repeat_interleave(2, 1), torch.cat([t[1], torch.full_like(t[1], float("nan"))], 1)]).contiguous()
                  for t in ts)
    twice_w = torch.stack([cx.repeat_interleave(2), torch.cat([wy, torch.zeros(n1, dtype=wy.dtype)])]).to(torch.uint8).cuda()
    ia, ib = _idx(0, 1), _idx(1, 0)
    for sim in SIMS:
        a, sa = eng.pair_score_weights(*ts, small_w, ia, ib, H, sim, return_status=True)
        b, sb = eng.pair_score_weights(*twice, twice_w, ia, ib, H, sim, return_status=True)
        assert sa.tolist() == sb.tolist() == [0, 0]
        gate = 2 * _gate(dtype, False, sim)
        for p in range(2):
            e = _score_err(float(a[p]), float(b[p]), sim, dtype)
            print(f"multiplicity D={D} {dtype} {sim} pair {p}: {float(a[p]):.8f} vs {float(b[p]):.8f} err {e:.3e} gate {gate:.1e}")
            assert e <= gate, (sim, p, float(a[p]), float(b[p]))


# ---- 4. invariance ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float16, 144, 2, 72), (torch.float32, 256, 4, 40)])
def test_batch_swap_and_self(eng, dtype, N, H, D):
    n = 5
    ts = _feats(n, 71, dtype, N, H, D)
    w = _weights(N, [N, 129 if N == 256 else 100, 64, 1, 33], 9)
    ia, ib = _idx(0, 1, 2, 3, 4), _idx(1, 2, 3, 4, 0)
    self_idx = torch.arange(n, dtype=torch.int32).cuda()
    for sim in SIMS:
        r1 = eng.pair_score_weights(*ts, w, ia, ib, H, sim)
        assert torch.isfinite(r1).all()
        for p in range(5):                                                                       # a pair alone == inside the batch of 5
            one = eng.pair_score_weights(*ts, w, ia[p:p + 1].clone(), ib[p:p + 1].clone(), H, sim)
            assert torch.equal(one[0], r1[p]), (sim, p)
        assert torch.equal(eng.pair_score_weights(*ts, w, ib, ia, H, sim), r1)                   # score(a, b) == score(b, a)
        own = eng.pair_score_weights(*ts, w, self_idx, self_idx, H, sim)                         # (a, a) with one weight row
        if sim == "mse":
            assert own.tolist() == [0.0] * n, own
        else:
            assert (own - 1.0).abs().max().item() <= _score_tol(dtype, False), own


@pytest.mark.parametrize("dtype,H,D", [(torch.bfloat16, 2, 160), (torch.float16, 2, 72), (torch.float32, 4, 40)])
def test_a_soft_region_scores_the_same_wherever_it_lies(eng, dtype, H, D):
    """The same rows with the same weights, in ascending order, at other token positions of N = 256: bit-identical scores."""
    N, sizes = 256, [100, 77, 130]
    g = torch.Generator().manual_seed(61)
    rows = [tuple((torch.randn(B, r, H * D, generator=g) * (0.5 + j)).to(dtype) for j in range(3)) for r in sizes]
    bytes_ = [torch.randint(1, 256, (r,), generator=g).to(torch.uint8) for r in sizes]
    ia, ib = _idx(0, 1, 2), _idx(1, 2, 0)

    def embed(seed):
        ts = tuple(torch.full_like(t, float("nan")) for t in _feats(3, seed, dtype, N, H, D))
        w = torch.zeros(3, N, dtype=torch.uint8)
        for i, pos in enumerate(_positions(N, sizes, seed)):
            w[i, pos] = bytes_[i]
            for t, x in zip(ts, rows[i]):
                t[i].index_copy_(1, pos.cuda(), x.cuda())
        return ts, w.cuda()
    for sim in SIMS:
        res = [eng.pair_score_weights(*ts, w, ia, ib, H, sim) for ts, w in (embed(1), embed(2))]
        assert torch.equal(res[0], res[1]) and torch.isfinite(res[0]).all(), (sim, res)


# ---- 5. an image without weight -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float32, 144, 2, 72), (torch.float16, 64, 4, 32)])
def test_an_image_without_weight_is_reported_and_leaves_the_others(eng, dtype, N, H, D):
    ts = _feats(3, 81, dtype, N, H, D)
    w = _weights(N, [N // 2, 40, 17], 4)
    ia, ib = _idx(0, 1, 2, 1), _idx(1, 2, 0, 1)
    for sim in SIMS:
        w2 = w.clone()
        w2[2] = 0
        got, st, sums = eng.pair_score_weights(*ts, w2, ia, ib, H, sim, return_status=True, return_sums=True)
        assert st.tolist() == [0, 2, 2, 0]
        assert torch.isnan(got[[1, 2]]).all()
        assert sums.tolist() == w2.long().sum(1).tolist() and sums[2].item() == 0
        without = eng.pair_score_weights(*(t[:2].contiguous() for t in ts), w[:2].contiguous(), _idx(0, 1), _idx(1, 1), H, sim)
        assert torch.equal(got[[0, 3]], without), (sim, got, without)


# ---- 6. refusals before enqueue -------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    from diffsim_amd import _lib
    L = _lib.lib()
    H, N, D = 4, 64, 32
    wsb = L.dsim_pair_score_weights_workspace_bytes
    need = int(wsb(3, 2, B, H, N, D))
    assert need > 0
    for args in ((0, 2, B, H, N, D), (3, 0, B, H, N, D), (3, 2, B, H, N, 24), (3, 2, B, H, N, 0), (3, 2, B, H, 0, D),
                 (3, 32768, B, H, N, D), (3, 2, 2, 32768, N, D), (3, 2, 0, H, N, D)):
        assert wsb(*args) == 0, args
    fake = ctypes.c_void_p(0x10000)                             # (never read: every refusal is decided on the host)

    def go(n_feat=3, n=2, H=H, N=N, D=D, dtype=_lib.DSIM_BF16, sim=0, ws=need):
        rc = L.dsim_pair_score_weights(fake, fake, fake, fake, n_feat, fake, fake, n, B, H, N, D, dtype, sim, fake, None, None, fake, ws,
                                       None)
        assert rc != 0
        return rc, L.dsim_strerror(rc).lower()

    assert b"workspace" in go(ws=need // 2)[1] and b"workspace" in go(ws=need - 257)[1]            # DSIM_ERR_WORKSPACE
    for kw in (dict(dtype=9), dict(dtype=-1), dict(sim=2), dict(sim=-1), dict(D=24), dict(D=0), dict(n=0), dict(n=-3), dict(n_feat=0)):
        for dtype in ((_lib.DSIM_BF16, _lib.DSIM_F16, _lib.DSIM_F32) if "dtype" not in kw else (kw["dtype"],)):
            assert b"invalid" in go(**{**kw, "dtype": dtype})[1], (kw, dtype)


# ---- 7. from files, tiny SD1.5 --------------------------------------------------------------------------------------------------------------
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


def _gray_mask_files(tmp_path, n, seed):
    """n grayscale mask images (60 x 44, mode L): blocks of 4 x 4 pixels that are black, white or a random gray, so that a token of
    any grid is partly covered"""
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    paths = []
    for i in range(n):
        kind = torch.randint(0, 3, (15, 11), generator=g)
        m = torch.where(kind == 0, 0, torch.where(kind == 1, 255, torch.randint(1, 255, (15, 11), generator=g))).to(torch.uint8)
        m[0, 0] = 255
        p = tmp_path / f"gray{seed}_{i}.png"
        Image.fromarray(m.repeat_interleave(4, 0).repeat_interleave(4, 1).numpy(), "L").save(p)
        paths.append(str(p))
    return paths


def _grid_mask_files(tmp_path, n, seed, grid):
    """n black-and-white mask images of 8 x 8 pixels per token of the grid: their area averages are 0 or 255"""
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    paths = []
    for i in range(n):
        m = (torch.rand(*grid, generator=g) < 0.5).to(torch.uint8) * 255
        m[0, 0] = 255
        p = tmp_path / f"bw{seed}_{i}.png"
        Image.fromarray(m.repeat_interleave(8, 0).repeat_interleave(8, 1).numpy(), "L").save(p)
        paths.append(str(p))
    return paths


def _sd15_tiny(dtype):
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.engine import VAEEncoder
    ctx = S.make_context(C.TINY)
    vae = VAEEncoder(C.VAE_TINY, S.make_state_dict(C.VAE_TINY, seed=3), torch.float32)
    return DiffSim(torch_dtype=dtype, device="cuda", unet_config=C.TINY, state_dict=S.make_state_dict(C.TINY, seed=0), vae=vae,
                   encode_prompt=lambda p: ctx)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sd15_tiny_soft_regions_from_files(eng, dtype, tmp_path):
    from diffsim_amd import config as C, harness as H, regions as R, textattn as TA
    from diffsim_amd.inputs import path_latents
    from diffsim_amd.scorer import stack_rows
    ds = _sd15_tiny(dtype)
    block, layer = "up_blocks", 0
    tap = ds.tap_of(block, layer)
    heads = ds.engine_at(tap).heads
    imgs, mks = _image_files(tmp_path, 4, 1), _gray_mask_files(tmp_path, 4, 2)
    pairs = [(imgs[0], imgs[1]), (imgs[2], imgs[3]), (imgs[1], imgs[0])]
    mpairs = [(mks[0], mks[1]), (mks[2], None), (mks[1], mks[0])]
    (latA, latB), nA, nB = path_latents(ds, pairs, (0, 1), 128, 2334, 16)
    grid = R.tap_grid(ds, tap, latA.shape[-1])
    N = grid[0] * grid[1]
    q, k, v = ds.tap_features(*stack_rows([latA.cuda(), latB.cuda()], [nA.cuda(), nB.cuda()], 0, 3), ds.bind_prompt("a cat", 3, "pairs"), tap,
                              600)
    rows = torch.stack([torch.stack([R.as_token_weights(m, grid).flatten() for m in mp]) for mp in mpairs]).reshape(6, N)
    assert 0 < int(((rows > 0) & (rows < 255)).sum())                               # partial coverage reached the grid
    ia = torch.arange(0, 6, 2, dtype=torch.int32).cuda()
    trip = [(imgs[0], imgs[1], imgs[2], "a cat"), (imgs[3], imgs[2], imgs[0], "a cat"), (imgs[1], imgs[3], imgs[2], "a cat")]
    tmasks = [(mks[0], mks[1], mks[2]), (None, mks[2], mks[0]), (mks[1], mks[3], None)]
    for sim in SIMS:
        # mask files -> weights -> the soft tail: the engine call on the same features, and float64
        got = R.score_path_pair_weights(ds, pairs, mpairs, 128, "a cat", block, layer, 600, 2334, sim)
        assert torch.equal(got, eng.pair_score_weights(q, k, v, rows.cuda(), ia, ia + 1, heads, sim)), sim
        want = soft64(q, k, v, rows, [0, 2, 4], [1, 3, 5], heads, sim, dtype)
        errs = [_score_err(float(got[p]), want[p], sim, dtype) for p in range(3)]
        print(f"sd15 tiny files {dtype} {sim}: errs {' '.join(f'{e:.3e}' for e in errs)} gate {_gate(dtype, False, sim):.1e}")
        assert max(errs) <= _gate(dtype, False, sim), (sim, got, want)
        # three triplets == six soft_region_score calls
        sl, sr, bad = H.score_path_triplets(ds, trip, 128, block, [0], 600, 2334, sim, batch_triplets=2, unet_triplets=2, masks=tmasks,
                                            soft=True)
        assert bad == 0
        for i, (t, m) in enumerate(zip(trip, tmasks)):
            wl = ds.soft_region_score(t[0], t[1], m[0], m[1], 128, "a cat", block, [0], 600, seed=2334, similarity=sim)
            wr = ds.soft_region_score(t[0], t[2], m[0], m[2], 128, "a cat", block, [0], 600, seed=2334, similarity=sim)
            assert wl.shape == (1,) and torch.equal(wl[0], sl[i]) and torch.equal(wr[0], sr[i]), (sim, i, wl, sl[i], wr, sr[i])
        # masks that are 0 / 255 on the grid: the region scores' bits, pairs and triplets
        bw = _grid_mask_files(tmp_path, 4, 3, grid)
        bpairs = [(bw[0], bw[1]), (bw[2], None), (bw[1], bw[0])]
        assert torch.equal(R.score_path_pair_weights(ds, pairs, bpairs, 128, "a cat", block, layer, 600, 2334, sim),
                           R.score_path_pair_regions(ds, pairs, bpairs, 128, "a cat", block, layer, 600, 2334, sim)), sim
        btm = [(bw[0], bw[1], bw[2]), (None, bw[2], bw[0]), (bw[1], bw[3], None)]
        hard = H.score_path_triplets(ds, trip, 128, block, [0], 600, 2334, sim, batch_triplets=2, unet_triplets=2, masks=btm)
        soft = H.score_path_triplets(ds, trip, 128, block, [0], 600, 2334, sim, batch_triplets=2, unet_triplets=2, masks=btm, soft=True)
        assert torch.equal(hard[0], soft[0]) and torch.equal(hard[1], soft[1]) and hard[2] == soft[2] == 0
        # soft text-guided regions: threshold 0 is the unmasked run, triplets and pairs
        w = torch.zeros(C.TINY.ctx_len)
        w[1:4] = 1.0
        plain = H.score_path_triplets(ds, trip, 128, block, [0], 600, 2334, sim, batch_triplets=2, unet_triplets=2)
        guide = TA.TextGuide(weights=w, rel_threshold=0.0, soft=True)
        zero = H.score_path_triplets(ds, trip, 128, block, [0], 600, 2334, sim, batch_triplets=2, unet_triplets=2, text=guide)
        assert torch.equal(zero[0], plain[0]) and torch.equal(zero[1], plain[1]) and guide.on_fraction == 1.0
        assert torch.equal(TA.score_latent_pairs_text(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, weights=w, rel_threshold=0.0,
                                                      soft=True),
                           ds.score_latent_pairs(latA, latB, nA, nB, "a cat", block, layer, 600, sim))
        # threshold 1: every hard-on token carries 255, the others their share; the scores are the soft tail's on those bytes
        _s, masks, _c = TA.score_latent_pairs_text(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, weights=w, batch_pairs=3,
                                                   return_regions=True)
        ts, bts, _c = TA.score_latent_pairs_text(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, weights=w, batch_pairs=3,
                                                 return_regions=True, soft=True)
        assert bts.dtype == torch.uint8 and bool((bts[masks.bool()] == 255).all())
        assert 0 < int(masks.sum()) < masks.numel() and bool((bts[~masks.bool()] < 255).any())
        want = soft64(q, k, v, bts.reshape(6, N), [0, 2, 4], [1, 3, 5], heads, sim, dtype)
        errs = [_score_err(float(ts[p]), want[p], sim, dtype) for p in range(3)]
        print(f"sd15 tiny text {dtype} {sim}: errs {' '.join(f'{e:.3e}' for e in errs)} gate {_gate(dtype, False, sim):.1e}")
        assert max(errs) <= _gate(dtype, False, sim), (sim, ts, want)
