"""Region maps (dsim_pair_score_maps_regions / engine.pair_score_maps_regions): the region score kept per query token, on the full
token grid.  Checked to the bit against pair_score_maps on physically compacted tensors and, with full masks, against pair_score_maps
itself; against the float64 restatement tests/_regionmap64.py; and for what the header promises: zeros at the off tokens, nothing
outside a region read, a region's position in the image irrelevant, a pair independent of its neighbours, an empty region reported.

Gates are the project's: the score's is test_gpu_regions._gate, the local map's test_gpu_maps.LOCAL_GATE (fp32: 1e-5 absolute, as
there), the sum of contrib and the agreement with pair_score_regions test_gpu_maps' 1e-6 max(1, |s|).
REGION_MAPS_FIRST_RUN below: the largest err / gate of the first MI355X run of test_unequal_regions_match_float64, per dtype
(recorded, not used)."""
import pytest
import torch

from tests._regionmap64 import region_maps64
from tests.test_gpu_maps import LOCAL_GATE, _local_err
from tests.test_gpu_regions import B, DTYPES, _compact, _feats, _gate, _idx, _masks, _score_err, _sizes

pytestmark = pytest.mark.gpu

# first MI355X run, largest err / gate over the cases of test_unequal_regions_match_float64 and the (1024, 8, 80) case: (score, local).
# Every gate held, so none was re-derived
REGION_MAPS_FIRST_RUN = {"float32": (0.006, 0.040), "bfloat16": (0.008, 0.368), "float16": (0.005, 0.407)}


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


def _rows(mask):
    return [torch.nonzero(m).flatten() for m in mask]


# ---- 1. pair_score_maps on compacted tensors, to the bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 63, 64, 65, 127, 128, 129, 255])
@pytest.mark.parametrize("D", [160, 40, 72])
@pytest.mark.parametrize("dtype", DTYPES)
def test_equals_the_maps_of_the_compacted_tensors(eng, dtype, D, r):
    """Two images with regions of r tokens at different positions inside N = 256: score, and local / contrib at the on tokens, are
    pair_score_maps' on the (n, B, r, H*D) tensors of the regions' rows, bit for bit; the off tokens hold exact zeros."""
    N, H = 256, 2
    ts = _feats(2, 100 + r + D, dtype, N, H, D)
    mask = _masks(N, [r, r], 7 * r + D)
    assert not torch.equal(mask[0], mask[1])
    rows = _rows(mask)
    comp = _compact(ts, mask)
    pairs = [(0, 1), (1, 0), (0, 0)]
    ia, ib = _idx(*(a for a, _ in pairs)), _idx(*(b for _, b in pairs))
    for sim in ("cosine", "mse"):
        score, local, contrib, st = eng.pair_score_maps_regions(*ts, mask, ia, ib, H, sim, return_status=True)
        ws, wl, wc, wst = eng.pair_score_maps(*comp, ia, ib, H, sim, return_status=True)
        assert torch.equal(score, ws), (sim, score, ws)
        assert torch.equal(st, wst) and st.tolist() == [0, 0, 0]
        for p, pr in enumerate(pairs):
            for d in range(2):
                on = rows[pr[d]]
                for got, want in ((local, wl), (contrib, wc)):
                    assert torch.equal(got[p, d, on], want[p, d]), (sim, p, d)
                    off = got[p, d][~mask[pr[d]]]
                    assert off.numel() == N - r and not off.any() and not torch.signbit(off).any()


# ---- 2. full regions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,D", [(256, 8, 160), (144, 2, 72), (196, 8, 72), (49, 2, 16)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_full_regions_are_the_similarity_maps(eng, dtype, N, H, D):
    ts = _feats(3, 21 + N + D, dtype, N, H, D)
    ia, ib = _idx(0, 1, 2, 1), _idx(1, 2, 0, 1)
    for mask in (torch.ones(3, N, dtype=torch.bool, device="cuda"), torch.full((3, N), 255, dtype=torch.uint8, device="cuda")):
        for sim in ("cosine", "mse"):
            got = eng.pair_score_maps_regions(*ts, mask, ia, ib, H, sim, return_status=True, return_counts=True)
            want = eng.pair_score_maps(*ts, ia, ib, H, sim, return_status=True)
            for g, w in zip(got[:4], want):
                assert torch.equal(g, w), sim
            assert got[3].tolist() == [0] * 4 and got[4].tolist() == [N] * 3


# ---- 3. float64, unequal regions ------------------------------------------------------------------------------------------------------
def _check64(eng, ts, mask, pairs, H, sim, dtype, peaked, label):
    """the checks of one float64 case; returns the largest (score err / gate, local err / gate)"""
    N = ts[0].shape[2]
    ia, ib = _idx(*(a for a, _ in pairs)), _idx(*(b for _, b in pairs))
    score, local, contrib, st = eng.pair_score_maps_regions(*ts, mask, ia, ib, H, sim, return_status=True)
    assert score.shape == (len(pairs),) and local.shape == contrib.shape == (len(pairs), 2, N)
    assert st.tolist() == [0] * len(pairs)
    want = region_maps64(*ts, mask, ia.cpu(), ib.cpu(), H, sim, dtype)
    region = eng.pair_score_regions(*ts, mask, ia, ib, H, sim)
    gate = _gate(dtype, peaked, sim)
    lgate = 1e-5 if dtype == torch.float32 else LOCAL_GATE[(dtype, sim)]
    worst_s = worst_l = 0.0
    msgs = []
    for p, (ws, wl, wc) in enumerate(want):
        gs = float(score[p])
        serr = _score_err(gs, ws, sim, dtype)
        gl = local[p].double().cpu()
        lerr = (gl - wl).abs().max().item() if dtype == torch.float32 else _local_err(gl, wl, sim)
        worst_s, worst_l = max(worst_s, serr / gate), max(worst_l, lerr / lgate)
        total = 0.5 * contrib[p].double().sum().item()
        if serr > gate:
            msgs.append(f"score pair {pairs[p]}: {gs} vs {ws}, err {serr:.3e} > {gate:.1e}")
        if lerr > lgate:
            msgs.append(f"local pair {pairs[p]}: err {lerr:.3e} > {lgate:.1e}")
        if abs(total - gs) > 1e-6 * max(1.0, abs(gs)):
            msgs.append(f"contrib sum pair {pairs[p]}: {total} vs {gs}")
        rs = float(region[p])
        if abs(gs - rs) > 1e-6 * max(1.0, abs(rs)):
            msgs.append(f"pair_score_regions pair {pairs[p]}: {gs} vs {rs}")
        for d in range(2):
            off = ~mask[pairs[p][d]]
            if local[p, d][off].any() or contrib[p, d][off].any():
                msgs.append(f"off tokens of pair {pairs[p]} direction {d} are not zero")
    print(f"{label} {str(dtype)[6:]} {sim} peaked={peaked}: score err/gate {worst_s:.3f} local err/gate {worst_l:.3f}")
    assert not msgs, msgs
    return worst_s, worst_l


@pytest.mark.parametrize("N,H,D", [(256, 8, 160), (256, 4, 40), (196, 8, 72), (64, 4, 32)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sim", ["cosine", "mse"])
@pytest.mark.parametrize("peaked", [False, True])
def test_unequal_regions_match_float64(eng, dtype, N, H, D, sim, peaked):
    """test_gpu_regions' case: four images with regions of N, about N/2, N/4 and 1 tokens, chained, and an image with itself; the
    features carry a channel mean for the reason given there."""
    ts = _feats(4, 41 + N + D, dtype, N, H, D, logit_scale=14.0 if peaked else 1.0, channel_mean=1.0)
    mask = _masks(N, _sizes(N), N + D)
    _check64(eng, ts, mask, [(0, 1), (1, 2), (2, 3), (3, 0), (1, 1)], H, sim, dtype, peaked, f"N={N} H={H} D={D}")


@pytest.mark.parametrize("sim", ["cosine", "mse"])
def test_several_query_tiles_and_early_leaving_workgroups_match_float64(eng, sim):
    """(1024, 8, 80) in bf16 with counts 700 and 130: six query tiles in one direction, two in the other, and the workgroups past
    them leave early"""
    N, H, D, dtype = 1024, 8, 80, torch.bfloat16
    ts = _feats(2, 43, dtype, N, H, D, channel_mean=1.0)
    mask = _masks(N, [700, 130], 17)
    _check64(eng, ts, mask, [(0, 1)], H, sim, dtype, False, f"N={N} H={H} D={D}")


# ---- 4. nothing outside a region is read into arithmetic ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 2, 160), (torch.float16, 200, 4, 40), (torch.float32, 144, 2, 72)])
def test_off_region_rows_are_never_read(eng, dtype, N, H, D):
    ts = _feats(3, 51, dtype, N, H, D)
    mask = _masks(N, [N // 2 + 1, 70, 33], 5)
    ia, ib = _idx(0, 1, 2), _idx(1, 2, 0)
    off = ~mask
    for sim in ("cosine", "mse"):
        clean = eng.pair_score_maps_regions(*ts, mask, ia, ib, H, sim)
        nan = tuple(t.clone() for t in ts)
        for t in nan:
            t.transpose(1, 2)[off] = float("nan")              # (n, N, B, HD) view: every off row of every CFG half
        assert not torch.isfinite(nan[0].float()).all()
        got = eng.pair_score_maps_regions(*nan, mask, ia, ib, H, sim, return_status=True)
        assert all(torch.equal(g, c) for g, c in zip(got[:3], clean)) and got[3].tolist() == [0, 0, 0], sim


# ---- 5. position invariance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,H,D", [(torch.bfloat16, 2, 160), (torch.float16, 2, 72), (torch.float32, 4, 40)])
def test_a_region_maps_the_same_wherever_it_lies(eng, dtype, H, D):
    """The same region rows, in ascending order, at other positions of N = 256 and of N = 512: bit-identical scores, and local and
    contrib bit-identical at corresponding tokens."""
    sizes = [100, 77, 130]
    g = torch.Generator().manual_seed(61)
    rows = [tuple((torch.randn(B, r, H * D, generator=g) * (0.5 + j)).to(dtype) for j in range(3)) for r in sizes]
    pairs = [(0, 1), (1, 2), (2, 0)]
    ia, ib = _idx(*(a for a, _ in pairs)), _idx(*(b for _, b in pairs))

    def embed(N, seed):
        mask = _masks(N, sizes, seed)
        ts = _feats(3, seed, dtype, N, H, D)
        for i in range(3):
            pos = torch.nonzero(mask[i]).flatten()
            for t, x in zip(ts, rows[i]):
                t[i].index_copy_(1, pos, x.cuda())
        return ts, mask
    for sim in ("cosine", "mse"):
        res = []
        for ts, mask in (embed(256, 1), embed(256, 2), embed(512, 3)):
            score, local, contrib = eng.pair_score_maps_regions(*ts, mask, ia, ib, H, sim)
            on = _rows(mask)
            res.append((score, [(local[p, d, on[pr[d]]], contrib[p, d, on[pr[d]]]) for p, pr in enumerate(pairs) for d in range(2)]))
        for other in res[1:]:
            assert torch.equal(res[0][0], other[0]), sim
            for (l0, c0), (l1, c1) in zip(res[0][1], other[1]):
                assert torch.equal(l0, l1) and torch.equal(c0, c1), sim
        assert torch.isfinite(res[0][0]).all()


# ---- 6. bit-level invariants ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float16, 144, 2, 72), (torch.float32, 256, 4, 40)])
def test_batch_repeat_swap_mask_byte_and_optional_outputs(eng, dtype, N, H, D):
    from diffsim_amd import _lib
    from diffsim_amd.engine import _TORCH2DSIM
    n = 6
    ts = _feats(n, 71, dtype, N, H, D)
    mask = _masks(N, [N, 129, 64, 1, 33, 100], 9)
    g = torch.Generator().manual_seed(3)
    ia = torch.randint(0, n, (16,), generator=g, dtype=torch.int32).cuda()
    ib = torch.randint(0, n, (16,), generator=g, dtype=torch.int32).cuda()
    for sim in ("cosine", "mse"):
        r1 = eng.pair_score_maps_regions(*ts, mask, ia, ib, H, sim)
        assert all(torch.equal(a, b) for a, b in zip(r1, eng.pair_score_maps_regions(*ts, mask, ia, ib, H, sim)))      # repeat calls
        for p in (0, 7, 15):                                                                     # a pair alone == inside the batch
            one = eng.pair_score_maps_regions(*ts, mask, ia[p:p + 1].clone(), ib[p:p + 1].clone(), H, sim)
            assert all(torch.equal(a[0], b[p]) for a, b in zip(one, r1)), (sim, p)
        sw = eng.pair_score_maps_regions(*ts, mask, ib, ia, H, sim)                              # swapping (a, b) swaps the directions
        assert torch.equal(sw[0], r1[0]) and torch.equal(sw[1], r1[1].flip(1)) and torch.equal(sw[2], r1[2].flip(1))
        for m in (mask.to(torch.uint8) * 255, mask.to(torch.uint8), mask.to(torch.uint8) * 7):   # any non-zero byte is on
            assert all(torch.equal(a, b) for a, b in zip(eng.pair_score_maps_regions(*ts, m, ia, ib, H, sim), r1))
        # local and contrib may be NULL, each on its own: the other outputs do not change
        L = _lib.lib()
        need = int(L.dsim_pair_score_maps_regions_workspace_bytes(n, 16, B, H, N, D))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        m8 = mask.view(torch.uint8)
        for want_local, want_contrib in ((False, False), (True, False), (False, True)):
            score = torch.full((16,), -7.0, device="cuda")
            lo = torch.full((16, 2, N), -7.0, device="cuda") if want_local else None
            co = torch.full((16, 2, N), -7.0, device="cuda") if want_contrib else None
            rc = L.dsim_pair_score_maps_regions(ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), m8.data_ptr(), n, ia.data_ptr(),
                                                ib.data_ptr(), 16, B, H, N, D, _TORCH2DSIM[dtype], 0 if sim == "cosine" else 1,
                                                score.data_ptr(), lo.data_ptr() if want_local else None,
                                                co.data_ptr() if want_contrib else None, None, None, ws.data_ptr(), need, None)
            torch.cuda.synchronize()
            assert rc == 0 and torch.equal(score, r1[0])
            assert lo is None or torch.equal(lo, r1[1])
            assert co is None or torch.equal(co, r1[2])


# ---- 7. empty region, non-finite features ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float32, 144, 2, 72), (torch.float16, 64, 4, 32)])
def test_an_empty_region_is_reported_and_leaves_the_others(eng, dtype, N, H, D):
    ts = _feats(4, 81, dtype, N, H, D)
    mask = _masks(N, [N // 2, 40, 17, N], 4)
    ia, ib = _idx(0, 1, 2, 3, 2), _idx(1, 2, 3, 0, 2)
    for sim in ("cosine", "mse"):
        clean = eng.pair_score_maps_regions(*ts, mask, ia, ib, H, sim, return_status=True)
        assert clean[3].tolist() == [0] * 5
        m2 = mask.clone()
        m2[2] = False
        score, local, contrib, st, cnt = eng.pair_score_maps_regions(*ts, m2, ia, ib, H, sim, return_status=True, return_counts=True)
        assert st.tolist() == [0, 2, 2, 0, 2] and cnt.tolist() == [N // 2, 40, 0, N]
        assert torch.isnan(score[[1, 2, 4]]).all()
        assert not local[[1, 2, 4]].any() and not contrib[[1, 2, 4]].any()
        for got, want in zip((score, local, contrib), clean):
            assert torch.equal(got[[0, 3]], want[[0, 3]])


@pytest.mark.parametrize("dtype,N,H,D", [(torch.float16, 256, 8, 160), (torch.float32, 144, 2, 72)])
def test_a_nan_feature_flags_exactly_its_pairs(eng, dtype, N, H, D):
    ts = _feats(4, 9, dtype, N, H, D)
    mask = _masks(N, [N // 2, 40, 90, 64], 6)
    ia, ib = _idx(0, 1, 2), _idx(1, 2, 3)
    clean = eng.pair_score_maps_regions(*ts, mask, ia, ib, H, "cosine", return_status=True)
    assert clean[3].tolist() == [0, 0, 0]
    k2 = ts[1].clone()
    k2[3, 1, int(torch.nonzero(mask[3])[5]), 5] = float("nan")          # an ON row of image 3
    got = eng.pair_score_maps_regions(ts[0], k2, ts[2], mask, ia, ib, H, "cosine", return_status=True)
    assert got[3].tolist() == [0, 0, 1]
    for a, b in zip(got[:3], clean[:3]):
        assert torch.equal(a[:2], b[:2])


# ---- 8. error codes ---------------------------------------------------------------------------------------------------------------------
def test_error_codes(eng):
    from diffsim_amd import _lib
    L = _lib.lib()
    N, H, D = 64, 4, 32
    q, k, v = _feats(2, 1, torch.bfloat16, N, H, D)
    mask = _masks(N, [30, 20], 1)
    m8 = mask.view(torch.uint8)
    ia, ib = _idx(0), _idx(1)
    with pytest.raises(_lib.DsimError):
        eng.pair_score_maps_regions(q, k, v, mask[:1], ia, ib, H)
    with pytest.raises(_lib.DsimError):
        eng.pair_score_maps_regions(q, k, v, mask.float(), ia, ib, H)
    with pytest.raises(_lib.DsimError):
        eng.pair_score_maps_regions(q, k.float(), v, mask, ia, ib, H)
    assert L.dsim_pair_score_maps_regions_workspace_bytes(2, 0, B, H, N, D) == 0
    assert L.dsim_pair_score_maps_regions_workspace_bytes(0, 1, B, H, N, D) == 0
    assert L.dsim_pair_score_maps_regions_workspace_bytes(2, 1, B, H, N, 24) == 0                 # an unserved head dim
    need = int(L.dsim_pair_score_maps_regions_workspace_bytes(2, 1, B, H, N, D))
    assert need >= 2 * N * 4 + 2 * 4 + 2 * 3 * B * H * N * 4
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty(1, device="cuda")

    def ptr(t):
        return None if t is None else t.data_ptr()

    def call(q_=q, mask_=m8, out_=out, d=D, ws_=ws, nbytes=need, n_feat=2):
        return L.dsim_pair_score_maps_regions(ptr(q_), k.data_ptr(), v.data_ptr(), ptr(mask_), n_feat, ia.data_ptr(), ib.data_ptr(), 1, B,
                                              H, N, d, _lib.DSIM_BF16, 0, ptr(out_), None, None, None, None, ptr(ws_), nbytes, None)
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, eng.pair_score_maps_regions(q, k, v, mask, ia, ib, H)[0])
    rc = call(nbytes=need // 2)
    assert rc != 0 and b"workspace" in L.dsim_strerror(rc).lower()
    for kw in ({"q_": None}, {"mask_": None}, {"out_": None}, {"ws_": None}, {"d": 24}, {"n_feat": 0}):
        rc = call(**kw)
        assert rc != 0 and b"invalid" in L.dsim_strerror(rc).lower(), kw


# ---- 9. end to end on synthetic weights -------------------------------------------------------------------------------------------------
def _close(a, b):
    """test_gpu_maps' gate between the maps and the pair path"""
    a, b = a.double().cpu(), b.double().cpu()
    return bool(((a - b).abs() <= 1e-6 * b.abs().clamp_min(1.0)).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sd15_tiny_region_maps_and_alignments_from_latents_and_files(eng, dtype, tmp_path):
    from diffsim_amd import align as AL, maps as M, regions as R
    from diffsim_amd.inputs import path_latents
    from diffsim_amd.scorer import stack_rows
    from tests.test_gpu_regions import _image_files, _mask_files, _sd15_tiny
    ds = _sd15_tiny(dtype)
    imgs, mks = _image_files(tmp_path, 4, 1), _mask_files(tmp_path, 4, 2)
    pairs = [(imgs[0], imgs[1]), (imgs[2], imgs[3]), (imgs[1], imgs[0])]
    (latA, latB), nA, nB = path_latents(ds, pairs, (0, 1), 128, 2334, 16)
    block, layer = "up_blocks", 0
    tap = ds.tap_of(block, layer)
    grid = R.tap_grid(ds, tap, latA.shape[-1])
    N = grid[0] * grid[1]
    g = torch.Generator().manual_seed(5)
    half_a, half_b = torch.rand(3, *grid, generator=g) < 0.5, torch.rand(3, N, generator=g) < 0.5
    half_a[:, 0, 0] = half_b[:, 0] = True
    heads = ds.engine_at(tap).heads
    q, k, v = ds.tap_features(*stack_rows([latA.cuda(), latB.cuda()], [nA.cuda(), nB.cuda()], 0, 3), ds.bind_prompt("a cat", 3, "pairs"), tap, 600)
    rows = torch.stack([half_a.flatten(1), half_b], 1).reshape(6, N).cuda()
    ia = torch.arange(0, 6, 2, dtype=torch.int32).cuda()
    for sim in ("cosine", "mse"):
        # latents and masks: the engine call on the same rows' features, and the region score
        mp = M.score_latent_pair_maps(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, batch_pairs=3, maskA=half_a, maskB=half_b)
        s, lo, co = eng.pair_score_maps_regions(q, k, v, rows, ia, ia + 1, heads, sim)
        assert torch.equal(mp.score, s) and torch.equal(mp.local.flatten(2), lo) and torch.equal(mp.contrib.flatten(2), co)
        assert torch.equal(mp.mask.flatten(2), rows.view(3, 2, N)) and not mp.local[~mp.mask].any()
        assert _close(mp.score, R.score_latent_pair_regions(ds, latA, latB, nA, nB, half_a, half_b, "a cat", block, layer, 600, sim))
        one = M.score_latent_pair_maps(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, batch_pairs=1, maskA=half_a, maskB=half_b)
        assert torch.equal(one.score, mp.score) and torch.equal(one.local, mp.local) and torch.equal(one.contrib, mp.contrib)
        assert torch.isfinite(mp.upsample(32)).all()
        # full masks: today's maps, to the bit
        full = torch.ones(3, N, dtype=torch.bool)
        fm = M.score_latent_pair_maps(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, maskA=full, maskB=full)
        pm = M.score_latent_pair_maps(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim)
        assert torch.equal(fm.score, pm.score) and torch.equal(fm.local, pm.local) and torch.equal(fm.contrib, pm.contrib) and pm.mask is None
    al = AL.score_latent_pair_alignment(ds, latA, latB, nA, nB, "a cat", block, layer, 600, batch_pairs=2, maskA=half_a, maskB=half_b)
    m, w, e = eng.pair_align_regions(q, k, rows, ia, ia + 1, heads, grid[1])
    assert torch.equal(al.match.flatten(2), m) and torch.equal(al.weight.flatten(2), w) and torch.equal(al.expect.flatten(2, 3), e)
    assert (al.match[~al.mask] == -1).all() and (al.match[al.mask] >= 0).all()
    fa = AL.score_latent_pair_alignment(ds, latA, latB, nA, nB, "a cat", block, layer, 600, maskA=torch.ones(3, N), maskB=torch.ones(3, N))
    pa = AL.score_latent_pair_alignment(ds, latA, latB, nA, nB, "a cat", block, layer, 600)
    assert torch.equal(fa.match, pa.match) and torch.equal(fa.weight, pa.weight) and torch.equal(fa.expect, pa.expect)
    # image and mask files: the scorer's methods against region_score
    mpairs = [(mks[0], mks[1]), (mks[2], None), (mks[1], mks[0])]
    for p, mk in zip(pairs, mpairs):
        want = ds.region_score(p[0], p[1], mk[0], mk[1], 128, "a cat", block, [0], 600, seed=2334, similarity="cosine")
        got = ds.region_similarity_maps(p[0], p[1], mk[0], mk[1], 128, "a cat", block, [0], 600, seed=2334, similarity="cosine")
        assert len(got) == 1 and _close(got.score, want), (got.score, want)
        assert torch.equal(got.mask[0, 0].cpu(), R.as_token_mask(mk[0], grid)) and torch.equal(got.mask[0, 1].cpu(), R.as_token_mask(mk[1], grid))
        assert _close(0.5 * got.contrib.double().sum((1, 2, 3)), got.score)
        ra = ds.region_alignment(p[0], p[1], mk[0], mk[1], 128, "a cat", block, [0], 600, seed=2334)
        assert torch.equal(ra.mask, got.mask) and (ra.match[~ra.mask] == -1).all()
        for d in range(2):                                                   # an on token points into the other image's region
            assert ra.mask[0, 1 - d].flatten()[ra.match[0, d][ra.mask[0, d]].long()].all()


def test_xl_and_dit_tiny_region_maps(tmp_path):
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim_dit import diffsim_DiT
    from diffsim_amd.diffsim_xl import diffsim_xl
    from tests._fakes import FakeVAE
    from tests.test_gpu_regions import _image_files, _mask_files
    a, b = _image_files(tmp_path, 2, 5)
    ma, mb = _mask_files(tmp_path, 2, 6)
    ctx, pooled = S.make_context(C.SDXL_TINY), S.make_pooled(C.SDXL_TINY)
    xl = diffsim_xl(torch.float32, "cuda", unet_config=C.SDXL_TINY, state_dict=S.make_state_dict(C.SDXL_TINY, seed=0), vae=FakeVAE(),
                    encode_prompt=lambda p: (ctx, pooled))
    dd = diffsim_DiT(128, 600, "cuda", dit_config=C.DIT_TINY, state_dict=S.make_state_dict(C.DIT_TINY, seed=0), vae=FakeVAE(),
                     torch_dtype=torch.float32)
    for sc, block, layer in ((xl, "up_blocks", [0, 1, 2]), (dd, "none", [2])):
        for sim in ("cosine", "mse"):
            want = sc.region_score(a, b, ma, mb, 128, "a cat", block, layer, 600, 2334, sim)
            got = sc.region_similarity_maps(a, b, ma, mb, 128, "a cat", block, layer, 600, 2334, sim)
            assert _close(got.score, want), (block, sim, got.score, want)
            assert not got.mask.all() and not got.local[~got.mask].any() and not got.contrib[~got.mask].any()
            whole = sc.region_similarity_maps(a, b, None, None, 128, "a cat", block, layer, 600, 2334, sim)
            plain = sc.similarity_maps(a, b, 128, "a cat", block, layer, 600, sim, 2334)
            assert whole.mask.all() and torch.equal(whole.score, plain.score) and torch.equal(whole.local, plain.local)
        ra = sc.region_alignment(a, b, ma, mb, 128, "a cat", block, layer, 600, 2334)
        assert torch.equal(ra.mask, got.mask) and (ra.match[~ra.mask] == -1).all() and (ra.match[ra.mask] >= 0).all()
        assert (ra.weight[ra.mask] > 0).all()


def test_text_guided_masks_fed_to_the_region_maps_reproduce_the_text_region_score():
    from diffsim_amd import config as C, maps as M, synth as S, textattn as TA
    from diffsim_amd.diffsim import DiffSim
    from tests import _textattn64 as X
    from tests._fakes import FakeVAE
    ctx = S.make_context(C.TINY)
    ds = DiffSim(torch_dtype=torch.float32, device="cuda", unet_config=C.TINY, state_dict=S.make_state_dict(C.TINY, seed=0), vae=FakeVAE(),
                 encode_prompt=lambda p: ctx)
    ds.tokenize = X.WordTokenizer(C.TINY.ctx_len)
    g = torch.Generator().manual_seed(11)
    lat, nz = torch.randn(4, 4, 16, 16, generator=g), torch.randn(4, 4, 16, 16, generator=g)
    latA, latB, nA, nB = lat[:3], lat[[1, 2, 3]], nz[:1], nz[1:2]
    for sim in ("cosine", "mse"):
        want, masks, counts = TA.score_latent_pairs_text(ds, latA, latB, nA, nB, "a cat", "up_blocks", 0, 600, sim, words=["cat"],
                                                         return_regions=True)
        N = masks.shape[-1]
        assert 0 < int(counts.min()) and int(counts.max()) < N               # regions, not whole images
        mp = M.score_latent_pair_maps(ds, latA, latB, nA, nB, "a cat", "up_blocks", 0, 600, sim, maskA=masks[:, 0], maskB=masks[:, 1])
        assert _close(mp.score, want), (sim, mp.score, want)
        assert torch.equal(mp.mask.flatten(2), masks.to(mp.mask.device))


def test_cli_writes_region_maps_and_matches_beside_the_rankings(tmp_path, monkeypatch, capsys):
    """--dataset retrieval with mask folders, --save_region_maps and --save_region_matches: one .npz and one .match.npz per query whose
    scores are the ranking file's, whose masks are the mask files on the token grid (a gallery image without one: whole)."""
    import numpy as np
    from diffsim_amd import cli, regions as R
    from tests.test_gpu_region_matrix import _image_files, _mask_file, _sd15_tiny
    ds = _sd15_tiny(torch.float32)
    qdir, gdir, qm, gm, out = (tmp_path / d for d in ("q", "g", "qm", "gm", "out"))
    for d in (qdir, gdir, qm, gm):
        d.mkdir()
    _image_files(qdir, 2, 11)
    gb = _image_files(gdir, 4, 12)
    qmasks = [_mask_file(qm / f"img11_{i}.png", 20 + i) for i in range(2)]
    gmasks = dict(zip(gb, [_mask_file(gm / f"img12_{i}.png", 30 + i) for i in range(3)] + [None]))
    monkeypatch.setattr(cli, "build_scorer", lambda args: ds)
    args = cli.arg_parse(["--dataset", "retrieval", "--query_path", str(qdir), "--image_path", str(gdir), "--out_path", str(out),
                          "--image_size", "128", "--target_block", "up_blocks", "--target_layer", "0", "--target_step", "600",
                          "--similarity", "cosine", "--topk", "3", "--query_mask_path", str(qm), "--gallery_mask_path", str(gm),
                          "--save_region_maps", "--save_region_matches"])
    assert cli.run(args) == 0
    text = capsys.readouterr().out
    assert "Region maps" in text and "Region alignments" in text
    for i, name in enumerate(("img11_0", "img11_1")):
        rank = [line.split() for line in open(out / f"{name}.txt").read().splitlines()]
        z, zm = np.load(out / f"{name}.npz"), np.load(out / f"{name}.match.npz")
        assert list(z["gallery"]) == [r[0] for r in rank] == list(zm["gallery"])
        for s, r in zip(z["score"].tolist(), rank):
            assert abs(s - float(r[1])) <= 1e-6 * max(1.0, abs(float(r[1]))), (name, s, r)
        grid = z["local"].shape[2:]
        assert z["mask"].shape == z["local"].shape == z["contrib"].shape == (3, 2, *grid) and z["mask"].dtype == np.bool_
        assert np.array_equal(z["mask"], zm["mask"]) and zm["match"].shape == (3, 2, *grid) and zm["expect"].shape == (3, 2, *grid, 2)
        for j, gpath in enumerate(z["gallery"]):
            assert np.array_equal(z["mask"][j, 0], R.as_token_mask(qmasks[i], grid).numpy())
            assert np.array_equal(z["mask"][j, 1], R.as_token_mask(gmasks[str(gpath)], grid).numpy())
        assert not z["local"][~z["mask"]].any() and (zm["match"][~zm["mask"]] == -1).all() and (zm["match"][zm["mask"]] >= 0).all()
        assert np.allclose(0.5 * z["contrib"].astype(np.float64).sum((1, 2, 3)), z["score"], rtol=0, atol=1e-6)
