"""Region scores (dsim_pair_score_regions / engine.pair_score_regions): the score tail restricted to a token region per image.
Checked to the bit against the pair tail on physically compacted tensors (the gather changes addresses and nothing else), against
the float64 restatement tests/_region64.py, and for what the header promises: nothing outside a region is read into arithmetic,
a region's position in the image does not matter, a pair does not depend on its neighbours, an empty region is reported.

Tolerances against float64 are test_gpu_maps.py's _score_tol / _score_err rule, restated here."""
import pytest
import torch

from tests._region64 import regions64

pytestmark = pytest.mark.gpu

B = 2
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


def _feats(n, seed, dtype, N, H, D, logit_scale=1.0, correlate=0.5, channel_mean=0.0):
    """test_gpu_maps.py's features: per image noise plus a part shared by the images token by token; channel_mean: plus a part of v
    shared by every token of every image, as the channel means of real features are"""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(n, B, N, H * D, generator=g) for _ in range(3))
    base = tuple(torch.randn(1, B, N, H * D, generator=g) for _ in range(3))
    q, k, v = (correlate * b + (1 - correlate) * t for b, t in zip(base, (q, k, v)))
    q = q * logit_scale
    if channel_mean:
        v = v + channel_mean * torch.randn(1, B, 1, H * D, generator=g)
    return tuple(t.to(dtype).cuda().contiguous() for t in (q, k, v))


def _idx(*xs):
    return torch.tensor(list(xs), dtype=torch.int32).cuda()


def _masks(N, sizes, seed):
    """(len(sizes), N) bool on the GPU: image i's region is sizes[i] tokens at seeded positions"""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(len(sizes), N, dtype=torch.bool)
    for i, r in enumerate(sizes):
        m[i, torch.randperm(N, generator=g)[:r]] = True
    return m.cuda()


def _compact(ts, mask):
    """the images' region rows in ascending order as tensors of their own, (n, B, r, H*D); every region has r tokens"""
    rows = [torch.nonzero(m).flatten() for m in mask]
    return tuple(torch.stack([t[i].index_select(1, rows[i]) for i in range(t.shape[0])]).contiguous() for t in ts)


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


# ---- 1. the pair tail on compacted tensors, to the bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 255])
@pytest.mark.parametrize("D", [160, 40, 72])
@pytest.mark.parametrize("dtype", DTYPES)
def test_equals_the_pair_tail_on_compacted_tensors(eng, dtype, D, r):
    """Two images with regions of r tokens at different positions inside N = 256: the region score is pair_score's (the tiled
    kernel: r != 256) on the (n, B, r, H*D) tensors of the regions' rows, score and status, bit for bit."""
    N, H = 256, 2
    ts = _feats(2, 100 + r + D, dtype, N, H, D)
    mask = _masks(N, [r, r], 7 * r + D)
    assert not torch.equal(mask[0], mask[1])
    cq, ck, cv = _compact(ts, mask)
    ia, ib = _idx(0, 1, 0), _idx(1, 0, 0)
    for sim in ("cosine", "mse"):
        got, st = eng.pair_score_regions(*ts, mask, ia, ib, H, sim, return_status=True)
        want, wst = eng.pair_score(cq, ck, cv, ia, ib, H, sim, return_status=True)
        assert torch.equal(got, want), (sim, got, want)
        assert torch.equal(st, wst) and st.tolist() == [0, 0, 0]


# ---- 2. full regions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.float32, 256, 8, 160), (torch.float32, 144, 2, 72), (torch.bfloat16, 256, 4, 40),
                                         (torch.float16, 144, 2, 72), (torch.bfloat16, 200, 2, 160), (torch.float16, 64, 4, 32)])
def test_full_regions_are_the_pair_score(eng, dtype, N, H, D):
    """(wherever pair_score is the tiled kernel: every shape but the 16-bit default tap)"""
    ts = _feats(3, 21 + N + D, dtype, N, H, D)
    ia, ib = _idx(0, 1, 2, 1), _idx(1, 2, 0, 1)
    for mask in (torch.ones(3, N, dtype=torch.bool, device="cuda"), torch.full((3, N), 255, dtype=torch.uint8, device="cuda")):
        for sim in ("cosine", "mse"):
            got, st, cnt = eng.pair_score_regions(*ts, mask, ia, ib, H, sim, return_status=True, return_counts=True)
            assert torch.equal(got, eng.pair_score(*ts, ia, ib, H, sim)), (sim, got)
            assert st.tolist() == [0] * 4 and cnt.tolist() == [N] * 3


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("sim", ["cosine", "mse"])
def test_full_regions_at_the_default_tap_match_float64(eng, dtype, sim):
    """(256, 8, 160) in 16 bits: pair_score is the persistent kernel there, the region score the tiled one; both against float64"""
    N, H, D = 256, 8, 160
    ts = _feats(3, 31, dtype, N, H, D)
    ia, ib = _idx(0, 1), _idx(1, 2)
    mask = torch.ones(3, N, dtype=torch.bool, device="cuda")
    got = eng.pair_score_regions(*ts, mask, ia, ib, H, sim)
    pair = eng.pair_score(*ts, ia, ib, H, sim)
    want = regions64(*ts, mask, ia.cpu(), ib.cpu(), H, sim, dtype)
    for p in range(2):
        print(f"default tap {dtype} {sim} pair {p}: region err {_score_err(float(got[p]), want[p], sim, dtype):.3e} "
              f"pair_score err {_score_err(float(pair[p]), want[p], sim, dtype):.3e}")
        assert _score_err(float(got[p]), want[p], sim, dtype) <= _gate(dtype, False, sim), (p, float(got[p]), want[p])
        assert _score_err(float(pair[p]), want[p], sim, dtype) <= _gate(dtype, False, sim), (p, float(pair[p]), want[p])


# ---- 3. float64, unequal regions ------------------------------------------------------------------------------------------------------
def _sizes(N):
    return [N, 129 if N == 256 else N // 2 + 1, 64 if N == 256 else N // 4, 1]


@pytest.mark.parametrize("N,H,D", [(256, 8, 160), (256, 4, 40), (144, 2, 72), (64, 4, 32)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sim", ["cosine", "mse"])
@pytest.mark.parametrize("peaked", [False, True])
def test_unequal_regions_match_float64(eng, dtype, N, H, D, sim, peaked):
    """Four images with regions of N, about N/2, N/4 and 1 tokens; the pairs chain them and (1, 1) is an image with itself.  The
    gates were set at N >= 64: for the pair whose regions are equal-sized, (1, 1), the pair tail on the compacted tensors is held
    to the same gate, which tells a small-region miss of the arithmetic from a gather bug.

    The values carry a channel mean (_feats): the fp32 gate is relative, and a relative gate on a cosine measures the kernel only
    where the cosine is away from zero.  Without it the one-token region's outputs are single, independent value rows, whose cosine
    is noise of size 1 / sqrt(B H D) around 0: there the f32 products' rounding (4.9e-9 absolute at (256, 8, 160), peaked, pair
    (2, 3), on the first MI355X run) read as 1.4e-5 relative."""
    ts = _feats(4, 41 + N + D, dtype, N, H, D, logit_scale=14.0 if peaked else 1.0, channel_mean=1.0)
    mask = _masks(N, _sizes(N), N + D)
    pairs = [(0, 1), (1, 2), (2, 3), (3, 0), (1, 1)]
    ia, ib = _idx(*(a for a, _ in pairs)), _idx(*(b for _, b in pairs))
    got, st, cnt = eng.pair_score_regions(*ts, mask, ia, ib, H, sim, return_status=True, return_counts=True)
    assert cnt.tolist() == _sizes(N) and st.tolist() == [0] * len(pairs)
    want = regions64(*ts, mask, ia.cpu(), ib.cpu(), H, sim, dtype)
    gate = _gate(dtype, peaked, sim)
    errs = [_score_err(float(got[p]), want[p], sim, dtype) for p in range(len(pairs))]
    one = _compact(tuple(t[1:2] for t in ts), mask[1:2])
    parent = float(eng.pair_score(*one, _idx(0), _idx(0), H, sim)[0])
    perr = _score_err(parent, want[4], sim, dtype)
    print(f"{dtype} N={N} H={H} D={D} {sim} peaked={peaked}: errs {' '.join(f'{e:.3e}' for e in errs)} parent(1,1) {perr:.3e} gate {gate:.1e}")
    assert perr <= gate, (parent, want[4])
    for p, e in enumerate(errs):
        assert e <= gate, (pairs[p], float(got[p]), want[p], e)


# ---- 4. nothing outside a region is read into arithmetic ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 2, 160), (torch.float16, 200, 4, 40), (torch.float32, 144, 2, 72)])
def test_off_region_rows_are_never_read(eng, dtype, N, H, D):
    ts = _feats(3, 51, dtype, N, H, D)
    mask = _masks(N, [N // 2 + 1, 70, 33], 5)
    ia, ib = _idx(0, 1, 2), _idx(1, 2, 0)
    off = ~mask
    for sim in ("cosine", "mse"):
        clean = eng.pair_score_regions(*ts, mask, ia, ib, H, sim)
        nan = tuple(t.clone() for t in ts)
        big = tuple(t.clone() for t in ts)
        for t in nan:
            t.transpose(1, 2)[off] = float("nan")              # (n, N, B, HD) view: every off row of every CFG half
        for j, t in enumerate(big):
            rows = t.transpose(1, 2)
            fill = torch.full_like(rows[off], 65504.0)
            fill[0::3] = float("inf")
            fill[1::3] = float("-inf")
            rows[off] = fill
        for bad in (nan, big):
            assert not torch.isfinite(bad[0].float()).all()
            got, st = eng.pair_score_regions(*bad, mask, ia, ib, H, sim, return_status=True)
            assert torch.equal(got, clean) and st.tolist() == [0, 0, 0], (sim, got, clean, st)


# ---- 5. position invariance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,H,D", [(torch.bfloat16, 2, 160), (torch.float16, 2, 72), (torch.float32, 4, 40)])
def test_a_region_scores_the_same_wherever_it_lies(eng, dtype, H, D):
    """The same region rows, in ascending order, at other positions of N = 256 and of N = 512: bit-identical scores."""
    sizes = [100, 77, 130]
    g = torch.Generator().manual_seed(61)
    rows = [tuple((torch.randn(B, r, H * D, generator=g) * (0.5 + j)).to(dtype) for j in range(3)) for r in sizes]
    ia, ib = _idx(0, 1, 2), _idx(1, 2, 0)

    def embed(N, seed):
        mask = _masks(N, sizes, seed)
        ts = _feats(3, seed, dtype, N, H, D)
        for i in range(3):
            pos = torch.nonzero(mask[i]).flatten()
            for t, x in zip(ts, rows[i]):
                t[i].index_copy_(1, pos, x.cuda())
        return ts, mask
    for sim in ("cosine", "mse"):
        res = [eng.pair_score_regions(*ts, mask, ia, ib, H, sim) for ts, mask in (embed(256, 1), embed(256, 2), embed(512, 3))]
        assert torch.equal(res[0], res[1]) and torch.equal(res[0], res[2]), (sim, res)
        assert torch.isfinite(res[0]).all()


# ---- 6. bit-level invariants ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float16, 144, 2, 72), (torch.float32, 256, 4, 40)])
def test_batch_repeat_swap_self_and_mask_byte(eng, dtype, N, H, D):
    n = 6
    ts = _feats(n, 71, dtype, N, H, D)
    mask = _masks(N, [N, 129, 64, 1, 33, 100], 9)
    g = torch.Generator().manual_seed(3)
    ia = torch.randint(0, n, (24,), generator=g, dtype=torch.int32).cuda()
    ib = torch.randint(0, n, (24,), generator=g, dtype=torch.int32).cuda()
    self_idx = torch.arange(n, dtype=torch.int32).cuda()
    for sim in ("cosine", "mse"):
        r1 = eng.pair_score_regions(*ts, mask, ia, ib, H, sim)
        assert torch.equal(r1, eng.pair_score_regions(*ts, mask, ia, ib, H, sim))                # repeat calls
        for p in range(24):                                                                      # a pair alone == inside the batch
            one = eng.pair_score_regions(*ts, mask, ia[p:p + 1].clone(), ib[p:p + 1].clone(), H, sim)
            assert torch.equal(one[0], r1[p]), (sim, p)
        assert torch.equal(eng.pair_score_regions(*ts, mask, ib, ia, H, sim), r1)                # swapped roles
        perm = torch.tensor([3, 0, 5, 1, 4, 2])                                                  # ... and images in another order
        inv = torch.argsort(perm).to(torch.int32).cuda()
        tp = tuple(t[perm.cuda()].contiguous() for t in ts)
        assert torch.equal(eng.pair_score_regions(*tp, mask[perm.cuda()].contiguous(), inv[ia.long()], inv[ib.long()], H, sim), r1)
        own = eng.pair_score_regions(*ts, mask, self_idx, self_idx, H, sim)                      # an image with itself over one region
        assert own.tolist() == [1.0 if sim == "cosine" else 0.0] * n, (sim, own)
        m255 = mask.to(torch.uint8) * 255
        m1 = mask.to(torch.uint8)
        assert torch.equal(eng.pair_score_regions(*ts, m255, ia, ib, H, sim), r1)
        assert torch.equal(eng.pair_score_regions(*ts, m1, ia, ib, H, sim), r1)


# ---- 7. empty region ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float32, 144, 2, 72), (torch.float16, 64, 4, 32)])
def test_an_empty_region_is_reported_and_leaves_the_others(eng, dtype, N, H, D):
    from diffsim_amd import _lib
    ts = _feats(4, 81, dtype, N, H, D)
    mask = _masks(N, [N // 2, 40, 17, N], 4)
    ia, ib = _idx(0, 1, 2, 3, 2), _idx(1, 2, 3, 0, 2)
    for sim in ("cosine", "mse"):
        clean, st0 = eng.pair_score_regions(*ts, mask, ia, ib, H, sim, return_status=True)
        assert st0.tolist() == [0] * 5
        m2 = mask.clone()
        m2[2] = False
        got, st, cnt = eng.pair_score_regions(*ts, m2, ia, ib, H, sim, return_status=True, return_counts=True)
        assert st.tolist() == [0, 2, 2, 0, 2]
        assert cnt.tolist() == [N // 2, 40, 0, N]
        assert torch.isnan(got[[1, 2, 4]]).all()
        assert torch.equal(got[[0, 3]], clean[[0, 3]])
    # the raw call: DSIM_OK with an empty region, status and counts NULL
    L = _lib.lib()
    need = L.dsim_pair_score_regions_workspace_bytes(4, 5, B, H, N, D)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty(5, device="cuda")
    m8 = m2.view(torch.uint8)
    args = (ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), m8.data_ptr(), 4, ia.data_ptr(), ib.data_ptr(), 5, B, H, N, D,
            {torch.float32: _lib.DSIM_F32, torch.bfloat16: _lib.DSIM_BF16, torch.float16: _lib.DSIM_F16}[dtype], 1, out.data_ptr(), None,
            None)
    assert L.dsim_pair_score_regions(*args, ws.data_ptr(), need, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[[0, 3]], got[[0, 3]]) and torch.isnan(out[[1, 2, 4]]).all()
    rc = L.dsim_pair_score_regions(*args, ws.data_ptr(), need // 2, None)
    assert rc != 0 and b"workspace" in L.dsim_strerror(rc).lower()


# ---- 8. end to end on synthetic weights -------------------------------------------------------------------------------------------------
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


def _mask_files(tmp_path, n, seed):
    """n mask images (64 x 48, mode L): random blocks, so that the token grids see whole, half and empty cells"""
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    paths = []
    for i in range(n):
        m = (torch.rand(8, 6, generator=g) < 0.5).to(torch.uint8) * 255
        m[0, 0] = 255
        p = tmp_path / f"mask{seed}_{i}.png"
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
def test_sd15_tiny_latent_path_and_triplet_regions(eng, dtype, tmp_path):
    from diffsim_amd import harness as H, regions as R
    ds = _sd15_tiny(dtype)
    imgs, mks = _image_files(tmp_path, 4, 1), _mask_files(tmp_path, 4, 2)
    pairs = [(imgs[0], imgs[1]), (imgs[2], imgs[3]), (imgs[1], imgs[0])]
    from diffsim_amd.inputs import path_latents
    (latA, latB), nA, nB = path_latents(ds, pairs, (0, 1), 128, 2334, 16)
    block, layer = "up_blocks", 0
    grid = R.tap_grid(ds, ds.tap_of(block, layer), latA.shape[-1])
    N = grid[0] * grid[1]
    full = torch.ones(3, N, dtype=torch.bool)
    g = torch.Generator().manual_seed(5)
    half_a, half_b = torch.rand(3, *grid, generator=g) < 0.5, torch.rand(3, N, generator=g) < 0.5
    half_a[:, 0, 0] = half_b[:, 0] = True
    for sim in ("cosine", "mse"):
        # full masks: the pair score (the tiny taps are the tiled kernel)
        got = R.score_latent_pair_regions(ds, latA, latB, nA, nB, full, full, "a cat", block, layer, 600, sim)
        assert torch.equal(got, ds.score_latent_pairs(latA, latB, nA, nB, "a cat", block, layer, 600, sim)), (sim, got)
        # half masks: the engine call on the same rows' features
        half = R.score_latent_pair_regions(ds, latA, latB, nA, nB, half_a, half_b, "a cat", block, layer, 600, sim, batch_pairs=3)
        from diffsim_amd.scorer import stack_rows
        q, k, v = ds.tap_features(*stack_rows([latA.cuda(), latB.cuda()], [nA.cuda(), nB.cuda()], 0, 3), ds.bind_prompt("a cat", 3, "pairs"),
                                  ds.tap_of(block, layer), 600)
        rows = torch.stack([half_a.flatten(1), half_b], 1).reshape(6, N).cuda()
        ia = torch.arange(0, 6, 2, dtype=torch.int32).cuda()
        assert torch.equal(half, eng.pair_score_regions(q, k, v, rows, ia, ia + 1, ds.engine_at(ds.tap_of(block, layer)).heads, sim))
        assert not torch.equal(half, got)
        one = R.score_latent_pair_regions(ds, latA, latB, nA, nB, half_a, half_b, "a cat", block, layer, 600, sim, batch_pairs=1)
        assert torch.equal(one, half)
    # image and mask files
    mpairs = [(mks[0], mks[1]), (mks[2], None), (mks[1], mks[0])]
    tm = [[R.as_token_mask(m, grid) for m in mp] for mp in mpairs]
    want = R.score_latent_pair_regions(ds, latA, latB, nA, nB, torch.stack([t[0] for t in tm]), torch.stack([t[1] for t in tm]), "a cat",
                                       block, layer, 600, "cosine")
    got = R.score_path_pair_regions(ds, pairs, mpairs, 128, "a cat", block, layer, 600, 2334, "cosine")
    assert torch.equal(got, want)
    for i, (p, m) in enumerate(zip(pairs, mpairs)):
        one = ds.region_score(p[0], p[1], m[0], m[1], 128, "a cat", block, [0], 600, seed=2334, similarity="cosine")
        assert one.shape == (1,) and torch.equal(one[0], want[i]), (i, one, want[i])
    # three triplets == six region_score calls
    trip = [(imgs[0], imgs[1], imgs[2], "a cat"), (imgs[3], imgs[2], imgs[0], "a cat"), (imgs[1], imgs[3], imgs[2], "a cat")]
    tmasks = [(mks[0], mks[1], mks[2]), (None, mks[2], mks[0]), (mks[1], mks[3], None)]
    sl, sr, bad = H.score_path_triplets(ds, trip, 128, block, [0], 600, 2334, "cosine", batch_triplets=2, unet_triplets=2, masks=tmasks)
    assert bad == 0
    for i, (t, m) in enumerate(zip(trip, tmasks)):
        wl = ds.region_score(t[0], t[1], m[0], m[1], 128, "a cat", block, [0], 600, seed=2334, similarity="cosine")
        wr = ds.region_score(t[0], t[2], m[0], m[2], 128, "a cat", block, [0], 600, seed=2334, similarity="cosine")
        assert torch.equal(wl[0], sl[i]) and torch.equal(wr[0], sr[i]), (i, wl, sl[i], wr, sr[i])


def test_xl_and_dit_tiny_region_scores(tmp_path):
    from diffsim_amd import config as C, regions as R, synth as S
    from diffsim_amd.diffsim_dit import diffsim_DiT
    from diffsim_amd.diffsim_xl import diffsim_xl
    from tests._fakes import FakeVAE
    a, b = _image_files(tmp_path, 2, 5)
    ma, mb = _mask_files(tmp_path, 2, 6)
    ctx, pooled = S.make_context(C.SDXL_TINY), S.make_pooled(C.SDXL_TINY)
    xl = diffsim_xl(torch.float32, "cuda", unet_config=C.SDXL_TINY, state_dict=S.make_state_dict(C.SDXL_TINY, seed=0), vae=FakeVAE(),
                    encode_prompt=lambda p: (ctx, pooled))
    dd = diffsim_DiT(128, 600, "cuda", dit_config=C.DIT_TINY, state_dict=S.make_state_dict(C.DIT_TINY, seed=0), vae=FakeVAE(),
                     torch_dtype=torch.float32)
    for sc, block, layer, score in ((xl, "up_blocks", [0, 1, 2], xl.diffsim_score), (dd, "none", [2], dd.diffsim_score)):
        for sim in ("cosine", "mse"):
            whole = sc.region_score(a, b, None, None, 128, "a cat", block, layer, 600, 2334, sim)
            assert whole.shape == (1,)
            assert torch.equal(whole.reshape(-1), score(a, b, 128, "a cat", block, layer, 600, sim, 2334).reshape(-1)), (block, sim)
            part = sc.region_score(a, b, ma, mb, 128, "a cat", block, layer, 600, 2334, sim)
            assert torch.isfinite(part).all() and not torch.equal(part, whole)
            grid = R.tap_grid(sc, sc.tap_of(block, layer), 16)
            again = sc.region_score(a, b, R.as_token_mask(ma, grid).numpy(), R.as_token_mask(mb, grid), 128, "a cat", block, layer, 600,
                                    2334, sim)
            assert torch.equal(again, part)
