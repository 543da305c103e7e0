"""Region score matrices (dsim_score_matrix_regions / engine.score_matrix_regions / retrieval's masks_a, masks_b): every image of
set A over its region against every image of set B over its region.  A cell is the region score of its pair, so it is checked to the
bit against engine.pair_score_regions over the same cells, against engine.score_matrix with full masks, against the float64
restatement tests/_region64.py, and for what the header promises: rows outside a region are never read, an empty region is
reported in its row and column alone, a cell does not depend on its neighbours, its set or where its region lies.

Tolerances against float64 are tests/test_gpu_regions.py's _score_tol / _score_err / _gate, restated here."""
import pytest
import torch

from tests._region64 import Region64

pytestmark = pytest.mark.gpu

B = 2
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


def _feats(n, seed, dtype, N, H, D, logit_scale=1.0, correlate=0.5, channel_mean=0.0):
    """tests/test_gpu_regions.py's features: per image noise plus a part shared by the images token by token; channel_mean: plus a
    part of v shared by every token of every image, as the channel means of real features are"""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(n, B, N, H * D, generator=g) for _ in range(3))
    base = tuple(torch.randn(1, B, N, H * D, generator=g) for _ in range(3))
    q, k, v = (correlate * b + (1 - correlate) * t for b, t in zip(base, (q, k, v)))
    q = q * logit_scale
    if channel_mean:
        v = v + channel_mean * torch.randn(1, B, 1, H * D, generator=g)
    return tuple(t.to(dtype).cuda().contiguous() for t in (q, k, v))


def _masks(N, sizes, seed):
    """(len(sizes), N) bool on the GPU: image i's region is sizes[i] tokens at seeded (scattered) positions"""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(len(sizes), N, dtype=torch.bool)
    for i, r in enumerate(sizes):
        m[i, torch.randperm(N, generator=g)[:r]] = True
    return m.cuda()


def _split(ts, mask, n_a):
    """the first n_a images as set A, the rest as set B: (fa, fb, mask_a, mask_b), each contiguous"""
    return (tuple(t[:n_a].contiguous() for t in ts), tuple(t[n_a:].contiguous() for t in ts), mask[:n_a].contiguous(),
            mask[n_a:].contiguous())


def _cells(n_a, n_b):
    """the pair indices of the n_a x n_b cells over the concatenated sets, row-major"""
    ia = torch.arange(n_a, dtype=torch.int32).repeat_interleave(n_b).cuda()
    ib = (n_a + torch.arange(n_b, dtype=torch.int32)).repeat(n_a).cuda()
    return ia, ib


# tests/test_gpu_regions.py: _score_tol, _score_err, _gate
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


# ---- 1. the region pair tail over the same cells, to the bit ------------------------------------------------------------------------
# seven different region sizes per shape (three query images, four gallery images), from {1, 31, 32, 33, 63, 64, 65, 127, 128, 129,
# 200, 255, N} clamped to N; every image of a matrix is a query in one direction and the keys in the other, and the three rows
# together hold every size of the set
SIZES = {(256, 2, 160): [1, 32, 63, 65, 128, 255, 256],
         (200, 4, 40): [31, 33, 64, 127, 129, 200, 1],
         (144, 2, 72): [144, 1, 32, 63, 64, 129, 33]}


def test_the_sizes_cover_the_boundaries():
    seen = {s for v in SIZES.values() for s in v}
    assert {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 255, 256, 144} <= seen
    assert all(len(set(v)) == 7 and max(v) <= shape[0] for shape, v in SIZES.items())


@pytest.mark.parametrize("N,H,D", list(SIZES))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sim", ["cosine", "mse"])
def test_equals_the_region_pair_tail(eng, dtype, N, H, D, sim):
    ts = _feats(7, 100 + N + D, dtype, N, H, D)
    mask = _masks(N, SIZES[(N, H, D)], N + D)
    fa, fb, ma, mb = _split(ts, mask, 3)
    got, st, cnt = eng.score_matrix_regions(fa, fb, ma, mb, H, sim, return_status=True, return_counts=True)
    want, wst = eng.pair_score_regions(*ts, mask, *_cells(3, 4), H, sim, return_status=True)
    assert cnt.tolist() == SIZES[(N, H, D)]
    assert torch.equal(got, want.view(3, 4)), (got, want)
    assert torch.equal(st, wst.view(3, 4)) and not st.any()


# ---- 2. full masks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.float32, 256, 2, 160), (torch.float32, 144, 2, 72), (torch.bfloat16, 256, 4, 40),
                                         (torch.float16, 256, 4, 40)])
def test_full_masks_are_the_score_matrix(eng, dtype, N, H, D):
    """(wherever score_matrix is the tiled kernel)"""
    ts = _feats(5, 21 + N + D, dtype, N, H, D)
    for full in (torch.ones(5, N, dtype=torch.bool, device="cuda"), torch.full((5, N), 255, dtype=torch.uint8, device="cuda")):
        fa, fb, ma, mb = _split(ts, full, 2)
        for sim in ("cosine", "mse"):
            got, st, cnt = eng.score_matrix_regions(fa, fb, ma, mb, H, sim, return_status=True, return_counts=True)
            want, wst = eng.score_matrix(fa, fb, H, sim, return_status=True)
            assert torch.equal(got, want), (sim, got, want)
            assert torch.equal(st, wst) and cnt.tolist() == [N] * 5


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("sim", ["cosine", "mse"])
def test_full_masks_at_the_default_tap_match_float64(eng, dtype, sim):
    """(256, 8, 160) in 16 bits: score_matrix is the persistent kernel there, the region matrix the tiled one; both against float64
    under tests/test_gpu_regions.py::test_full_regions_at_the_default_tap_match_float64's gate, _gate(dtype, False, sim)"""
    N, H, D = 256, 8, 160
    ts = _feats(4, 31, dtype, N, H, D)
    full = torch.ones(4, N, dtype=torch.bool, device="cuda")
    fa, fb, ma, mb = _split(ts, full, 2)
    got = eng.score_matrix_regions(fa, fb, ma, mb, H, sim)
    mat = eng.score_matrix(fa, fb, H, sim)
    r64 = Region64(*ts, full, H, dtype)
    for i in range(2):
        for j in range(2):
            want = r64.pair(i, 2 + j, sim)
            e_r, e_m = _score_err(float(got[i, j]), want, sim, dtype), _score_err(float(mat[i, j]), want, sim, dtype)
            print(f"default tap {dtype} {sim} cell ({i}, {j}): region matrix err {e_r:.3e} score_matrix err {e_m:.3e}")
            assert e_r <= _gate(dtype, False, sim), (i, j, float(got[i, j]), want)
            assert e_m <= _gate(dtype, False, sim), (i, j, float(mat[i, j]), want)


# ---- 3. float64, unequal regions ----------------------------------------------------------------------------------------------------
def _sizes(N):
    """tests/test_gpu_regions.py's: N, about N/2, N/4 and one token -- here set A holds the first and the third, set B the others"""
    return [N, 64 if N == 256 else N // 4, 129 if N == 256 else N // 2 + 1, 1]


@pytest.mark.parametrize("N,H,D", [(256, 8, 160), (256, 4, 40), (144, 2, 72), (64, 4, 32)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sim", ["cosine", "mse"])
@pytest.mark.parametrize("peaked", [False, True])
def test_unequal_regions_match_float64(eng, dtype, N, H, D, sim, peaked):
    """The gates are tests/test_gpu_regions.py::test_unequal_regions_match_float64's, _gate(dtype, peaked, sim), and the features
    carry a channel mean for the reason that test gives: a relative gate on a cosine measures the kernel only where the cosine is
    away from zero."""
    ts = _feats(4, 41 + N + D, dtype, N, H, D, logit_scale=14.0 if peaked else 1.0, channel_mean=1.0)
    mask = _masks(N, _sizes(N), N + D)
    fa, fb, ma, mb = _split(ts, mask, 2)
    got, st, cnt = eng.score_matrix_regions(fa, fb, ma, mb, H, sim, return_status=True, return_counts=True)
    assert cnt.tolist() == _sizes(N) and not st.any()
    r64 = Region64(*ts, mask, H, dtype)
    gate = _gate(dtype, peaked, sim)
    errs = {(i, j): _score_err(float(got[i, j]), r64.pair(i, 2 + j, sim), sim, dtype) for i in range(2) for j in range(2)}
    print(f"{dtype} N={N} H={H} D={D} {sim} peaked={peaked}: errs {' '.join(f'{e:.3e}' for e in errs.values())} gate {gate:.1e}")
    for c, e in errs.items():
        assert e <= gate, (c, float(got[c]), e)


# ---- 4. nothing outside a region is read into arithmetic ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 2, 160), (torch.float16, 200, 4, 40), (torch.float32, 144, 2, 72)])
def test_off_region_rows_are_never_read(eng, dtype, N, H, D):
    ts = _feats(5, 51, dtype, N, H, D)
    mask = _masks(N, [N // 2 + 1, 70, 33, 129, 1], 5)
    off = ~mask
    fa, fb, ma, mb = _split(ts, mask, 2)
    for sim in ("cosine", "mse"):
        clean = eng.score_matrix_regions(fa, fb, ma, mb, H, sim)
        nan = tuple(t.clone() for t in ts)
        big = tuple(t.clone() for t in ts)
        for t in nan:
            t.transpose(1, 2)[off] = float("nan")              # (n, N, B, HD) view: every off row of every CFG half
        for t in big:
            rows = t.transpose(1, 2)
            fill = torch.full_like(rows[off], 65504.0)
            fill[0::3] = float("inf")
            fill[1::3] = float("-inf")
            rows[off] = fill
        for bad in (nan, big):
            assert not torch.isfinite(bad[0].float()).all()
            ba, bb, _, _ = _split(bad, mask, 2)
            got, st = eng.score_matrix_regions(ba, bb, ma, mb, H, sim, return_status=True)
            assert torch.equal(got, clean) and not st.any(), (sim, got, clean, st)


# ---- 5. empty regions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float32, 144, 2, 72), (torch.float16, 64, 4, 32)])
def test_empty_regions_are_reported_in_their_row_and_column_alone(eng, dtype, N, H, D):
    ts = _feats(7, 81, dtype, N, H, D)
    sizes = [N // 2, 0, 40, 17, N, 0, 33]                      # query 1 and gallery image 2 (index 5) are empty
    mask = _masks(N, sizes, 4)
    fa, fb, ma, mb = _split(ts, mask, 3)
    keep_a, keep_b = torch.tensor([0, 2]).cuda(), torch.tensor([0, 1, 3]).cuda()
    for sim in ("cosine", "mse"):
        got, st, cnt = eng.score_matrix_regions(fa, fb, ma, mb, H, sim, return_status=True, return_counts=True)
        assert cnt.tolist() == sizes
        want_st = torch.zeros(3, 4, dtype=torch.int32)
        want_st[1, :] = 2
        want_st[:, 2] = 2
        assert torch.equal(st.cpu(), want_st)
        assert torch.isnan(got[1, :]).all() and torch.isnan(got[:, 2]).all()
        ga, gb = tuple(t[keep_a].contiguous() for t in fa), tuple(t[keep_b].contiguous() for t in fb)
        clean, cst = eng.score_matrix_regions(ga, gb, ma[keep_a].contiguous(), mb[keep_b].contiguous(), H, sim, return_status=True)
        assert not cst.any() and torch.isfinite(clean).all()
        assert torch.equal(got[keep_a][:, keep_b], clean), (sim, got, clean)
    # every image empty: the call itself is fine
    none = torch.zeros_like(mask)
    got, st = eng.score_matrix_regions(fa, fb, none[:3].contiguous(), none[3:].contiguous(), H, "cosine", return_status=True)
    assert torch.isnan(got).all() and (st == 2).all()


# ---- 6. independence and symmetry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float16, 144, 2, 72), (torch.float32, 256, 4, 40)])
def test_alone_repeat_streams_transpose_and_self(eng, dtype, N, H, D):
    ts = _feats(6, 71, dtype, N, H, D)
    mask = _masks(N, [N, 129, 64, 1, 33, 100], 9)
    fa, fb, ma, mb = _split(ts, mask, 2)
    for sim in ("cosine", "mse"):
        r1 = eng.score_matrix_regions(fa, fb, ma, mb, H, sim)
        assert torch.equal(r1, eng.score_matrix_regions(fa, fb, ma, mb, H, sim))                          # a repeat call
        for i in range(2):                                                                                  # a cell alone
            for j in range(4):
                one = eng.score_matrix_regions(tuple(t[i:i + 1] for t in fa), tuple(t[j:j + 1] for t in fb), ma[i:i + 1], mb[j:j + 1], H, sim)
                assert torch.equal(one[0, 0], r1[i, j]), (sim, i, j)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]                                                # two streams
        torch.cuda.synchronize()
        res = []
        for s in streams:
            with torch.cuda.stream(s):
                res.append(eng.score_matrix_regions(fa, fb, ma, mb, H, sim))
        torch.cuda.synchronize()
        assert torch.equal(res[0], r1) and torch.equal(res[1], r1)
        assert torch.equal(eng.score_matrix_regions(fb, fa, mb, ma, H, sim).T, r1)                        # the sets swapped
        m255 = mask.to(torch.uint8) * 255                                                                   # any non-zero byte is on
        assert torch.equal(eng.score_matrix_regions(fa, fb, m255[:2].contiguous(), m255[2:].contiguous(), H, sim), r1)
        own = eng.score_matrix_regions(ts, ts, mask, mask, H, sim)                                        # an image in both sets
        assert own.diagonal().tolist() == [1.0 if sim == "cosine" else 0.0] * 6, (sim, own.diagonal())
        assert torch.equal(own, own.T)
        assert torch.equal(own[:2, 2:], r1)                                                                 # ... and a cell in a bigger matrix


@pytest.mark.parametrize("dtype,H,D", [(torch.bfloat16, 2, 160), (torch.float16, 2, 72), (torch.float32, 4, 40)])
def test_a_region_scores_the_same_wherever_it_lies(eng, dtype, H, D):
    """The same region rows, in ascending order, at other positions of N = 256 and of N = 512: bit-identical cells."""
    sizes = [100, 77, 130, 33]
    g = torch.Generator().manual_seed(61)
    rows = [tuple((torch.randn(B, r, H * D, generator=g) * (0.5 + j)).to(dtype) for j in range(3)) for r in sizes]

    def embed(N, seed):
        mask = _masks(N, sizes, seed)
        ts = _feats(4, seed, dtype, N, H, D)
        for i in range(4):
            pos = torch.nonzero(mask[i]).flatten()
            for t, x in zip(ts, rows[i]):
                t[i].index_copy_(1, pos, x.cuda())
        return _split(ts, mask, 2)
    for sim in ("cosine", "mse"):
        res = [eng.score_matrix_regions(*e, H, sim) for e in (embed(256, 1), embed(256, 2), embed(512, 3))]
        assert torch.equal(res[0], res[1]) and torch.equal(res[0], res[2]), (sim, res)
        assert torch.isfinite(res[0]).all()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(eng):
    """DSIM_ERR_WORKSPACE for a workspace one byte short of what the launcher needs (the query's answer less its 256 bytes of
    alignment slack; the pointer here is aligned), DSIM_ERR_INVALID with a workspace query of 0 for n_a = 0, a head dim outside the
    set and a bad dtype; the output keeps its bytes in every case."""
    from diffsim_amd import _lib
    L = _lib.lib()
    OK, INVALID, WORKSPACE = 0, -1, -3                          # include/diffsim_amd.h: DSIM_OK, DSIM_ERR_INVALID, DSIM_ERR_WORKSPACE
    N, H, D = 64, 4, 32
    ts = _feats(3, 91, torch.bfloat16, N, H, D)
    mask = _masks(N, [N, 20, 7], 1).view(torch.uint8)
    query = L.dsim_score_matrix_regions_workspace_bytes
    need = int(query(1, 2, B, H, N, D, _lib.DSIM_BF16))
    assert need > 256
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    out = torch.full((2,), -7.0, device="cuda")

    def call(n_a=1, D_=D, dtype=_lib.DSIM_BF16, wsb=need):
        rc = L.dsim_score_matrix_regions(ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), mask.data_ptr(), n_a,
                                         ts[0][1:].data_ptr(), ts[1][1:].data_ptr(), ts[2][1:].data_ptr(), mask[1:].data_ptr(), 2, B, H, N, D_,
                                         dtype, 0, out.data_ptr(), None, None, ws.data_ptr(), wsb, None)
        torch.cuda.synchronize()
        return rc
    assert call(wsb=need - 257) == WORKSPACE
    assert call(n_a=0) == INVALID and query(0, 2, B, H, N, D, _lib.DSIM_BF16) == 0
    assert call(D_=24) == INVALID and query(1, 2, B, H, N, 24, _lib.DSIM_BF16) == 0
    assert call(dtype=9) == INVALID and query(1, 2, B, H, N, D, 9) == 0
    assert out.tolist() == [-7.0, -7.0]
    assert call(wsb=need - 256) == OK                # the same call with the workspace it needs
    want = eng.score_matrix_regions(tuple(t[:1] for t in ts), tuple(t[1:] for t in ts), mask[:1], mask[1:], H)
    assert torch.equal(out, want[0])


# ---- 8. through the scorers -----------------------------------------------------------------------------------------------------------
def _image_files(folder, n, seed):
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    paths = []
    for i in range(n):
        base = torch.rand(3, 1, 1, generator=g) * 255
        px = (base + 60 * torch.randn(3, 160, 144, generator=g)).clamp(0, 255).to(torch.uint8)
        p = folder / f"img{seed}_{i}.png"
        Image.fromarray(px.permute(1, 2, 0).numpy()).save(p)
        paths.append(str(p))
    return paths


def _mask_file(path, seed):
    """a mask image (64 x 48, mode L) of random blocks, so that the token grids see whole, half and empty cells"""
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(8, 6, generator=g) < 0.5).to(torch.uint8) * 255
    m[0, 0] = 255
    Image.fromarray(m.repeat_interleave(8, 0).repeat_interleave(8, 1).numpy(), "L").save(path)
    return str(path)


def _sd15_tiny(dtype):
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.engine import VAEEncoder
    ctx = S.make_context(C.TINY)
    vae = VAEEncoder(C.VAE_TINY, S.make_state_dict(C.VAE_TINY, seed=3), torch.float32)
    return DiffSim(torch_dtype=dtype, device="cuda", unet_config=C.TINY, state_dict=S.make_state_dict(C.TINY, seed=0), vae=vae,
                   encode_prompt=lambda p: ctx)


def _half_masks(n, grid, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(n, *grid, generator=g) < 0.5
    m[:, 0, 0] = True
    return m


def _pair_cells(R, sc, latA, latB, nA, nB, mA, mB, prompt, block, layer, sim):
    """regions.score_latent_pair_regions over the n_a x n_b cells, as (n_a, n_b)"""
    n_a, n_b = latA.shape[0], latB.shape[0]
    s = R.score_latent_pair_regions(sc, latA.repeat_interleave(n_b, 0), latB.repeat(n_a, 1, 1, 1), nA, nB, mA.repeat_interleave(n_b, 0),
                                    mB.repeat(n_a, *([1] * (mB.ndim - 1))), prompt, block, layer, 600, sim)
    return s.view(n_a, n_b)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sd15_tiny_latent_matrix_equals_the_region_pairs(dtype, tmp_path):
    from diffsim_amd import regions as R
    from diffsim_amd.inputs import path_latents
    from diffsim_amd.retrieval import score_latent_matrix
    ds = _sd15_tiny(dtype)
    qa, gb = _image_files(tmp_path, 3, 1), _image_files(tmp_path, 3, 2)
    (latA,), nA, _ = path_latents(ds, [(p,) for p in qa], (0,), 128, 2334, 16)
    (latB,), _, nB = path_latents(ds, [(p,) for p in gb], (1,), 128, 2334, 16)
    block, layer = "up_blocks", 0
    grid = R.tap_grid(ds, ds.tap_of(block, layer), latA.shape[-1])
    mA, mB = _half_masks(3, grid, 5), _half_masks(3, grid, 6)
    full = torch.ones(3, *grid, dtype=torch.bool)
    for sim in ("cosine", "mse"):
        m = score_latent_matrix(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, masks_a=mA, masks_b=mB)
        assert torch.equal(m, _pair_cells(R, ds, latA, latB, nA, nB, mA, mB, "a cat", block, layer, sim)), (sim, m)
        two = score_latent_matrix(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, batch=2, masks_a=mA, masks_b=mB)
        assert torch.equal(two, m)                                                           # two gallery chunks
        only_a = score_latent_matrix(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, masks_a=mA)
        assert torch.equal(only_a, score_latent_matrix(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, masks_a=mA, masks_b=full))
        assert not torch.equal(only_a, m)
        whole = score_latent_matrix(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, masks_a=full, masks_b=list(full.flatten(1)))
        assert torch.equal(whole, score_latent_matrix(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim))


def test_xl_and_dit_tiny_region_matrices(tmp_path):
    from diffsim_amd import config as C, regions as R, synth as S
    from diffsim_amd.diffsim_dit import diffsim_DiT
    from diffsim_amd.diffsim_xl import diffsim_xl
    from diffsim_amd.inputs import path_latents
    from diffsim_amd.retrieval import score_latent_matrix
    from tests._fakes import FakeVAE
    qa, gb = _image_files(tmp_path, 2, 5), _image_files(tmp_path, 3, 6)
    ctx, pooled = S.make_context(C.SDXL_TINY), S.make_pooled(C.SDXL_TINY)
    xl = diffsim_xl(torch.float32, "cuda", unet_config=C.SDXL_TINY, state_dict=S.make_state_dict(C.SDXL_TINY, seed=0), vae=FakeVAE(),
                    encode_prompt=lambda p: (ctx, pooled))
    dd = diffsim_DiT(128, 600, "cuda", dit_config=C.DIT_TINY, state_dict=S.make_state_dict(C.DIT_TINY, seed=0), vae=FakeVAE(),
                     torch_dtype=torch.float32)
    for sc, block, layer in ((xl, "up_blocks", [0, 1, 2]), (dd, "none", [2])):
        (latA,), nA, _ = path_latents(sc, [(p,) for p in qa], (0,), 128, 2334, 16)
        (latB,), _, nB = path_latents(sc, [(p,) for p in gb], (1,), 128, 2334, 16)
        grid = R.tap_grid(sc, sc.tap_of(block, layer), latA.shape[-1])
        mA, mB = _half_masks(2, grid, 7), _half_masks(3, grid, 8)
        m = score_latent_matrix(sc, latA, latB, nA, nB, "a cat", block, layer, 600, "cosine", masks_a=mA, masks_b=mB)
        assert torch.equal(m, _pair_cells(R, sc, latA, latB, nA, nB, mA, mB, "a cat", block, layer, "cosine")), (block, m)
        assert not torch.equal(m, score_latent_matrix(sc, latA, latB, nA, nB, "a cat", block, layer, 600, "cosine"))


def test_cli_ranks_by_the_masked_regions(tmp_path, monkeypatch, capsys):
    """--dataset retrieval --query_mask_path --gallery_mask_path on generated images and mask folders (one gallery image has no mask
    file): the ranking files are retrieval.topk of score_path_matrix with the same masks."""
    from diffsim_amd import cli, retrieval
    ds = _sd15_tiny(torch.float32)
    qdir, gdir, qm, gm, out = (tmp_path / d for d in ("q", "g", "qm", "gm", "out"))
    for d in (qdir, gdir, qm, gm):
        d.mkdir()
    qa, gb = _image_files(qdir, 2, 11), _image_files(gdir, 4, 12)
    qmasks = [_mask_file(qm / f"img11_{i}.png", 20 + i) for i in range(2)]
    gmasks = [_mask_file(gm / f"img12_{i}.png", 30 + i) for i in range(3)] + [None]
    monkeypatch.setattr(cli, "build_scorer", lambda args: ds)
    args = cli.arg_parse(["--dataset", "retrieval", "--query_path", str(qdir), "--image_path", str(gdir), "--out_path", str(out),
                          "--image_size", "128", "--target_block", "up_blocks", "--target_layer", "0", "--target_step", "600",
                          "--similarity", "cosine", "--topk", "3", "--query_mask_path", str(qm), "--gallery_mask_path", str(gm)])
    assert cli.run(args) == 0
    assert "1 image(s) without a mask file" in capsys.readouterr().out
    m = retrieval.score_path_matrix(ds, qa, gb, 128, args.prompt, "up_blocks", 0, 600, args.seed, "cosine", masks_a=qmasks, masks_b=gmasks)
    assert not torch.equal(m, retrieval.score_path_matrix(ds, qa, gb, 128, args.prompt, "up_blocks", 0, 600, args.seed, "cosine"))
    vals, idx = retrieval.topk(m, 3, "cosine")
    for i, name in enumerate(("img11_0", "img11_1")):
        rank = [l.split() for l in open(out / f"{name}.txt").read().splitlines()]
        assert [r[0] for r in rank] == [gb[j] for j in idx[i].tolist()]
        assert [float(r[1]) for r in rank] == [float(f"{v:.8g}") for v in vals[i].tolist()]
