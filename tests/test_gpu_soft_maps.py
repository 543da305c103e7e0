"""Soft region maps (dsim_pair_score_maps_weights / engine.pair_score_maps_weights): the soft region score per query token.  Checked
to the bit against engine.pair_score_maps_regions where every byte is 0 or 255, against the float64 restatement
tests/_softmap64.py for general bytes (score, local, the contrib sum, agreement with engine.pair_score_weights, exact zeros at
weight 0), and for what the header promises: weights are multiplicities, a pair depends on its two images and their weights alone,
an image without weight is reported, a NaN feature flags exactly its pairs.

Features, weights and gates are tests/test_gpu_soft_regions.py's (_feats, _weights, _poison, _sizes, _gate, _score_err); the gate of
`local` is tests/test_gpu_maps.py's LOCAL_GATE / _local_err (1e-5 absolute in fp32, as tests/test_gpu_region_maps.py); the contrib
sum and the agreement with pair_score_weights are held to 1e-6 max(1, |s|).

Recorded, not used -- the first MI355X run's largest err / gate per dtype over test_general_bytes_match_float64 and
test_several_query_tiles_and_early_leaving_workgroups:

    dtype      score err / gate    local err / gate
    float32    0.006              0.013
    bfloat16   0.007              0.295
    float16    0.007              0.481
"""
import pytest
import torch

from tests._softmap64 import soft_maps64
from tests.test_gpu_maps import LOCAL_GATE, _local_err
from tests.test_gpu_soft_regions import B, DTYPES, SIMS, _feats, _gate, _idx, _poison, _score_err, _sizes, _weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


# ---- 1. bytes 0 / 255 are the region maps, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 63, 64, 65, 127, 128, 129, 255])
@pytest.mark.parametrize("D", [160, 40, 72])
@pytest.mark.parametrize("dtype", DTYPES)
def test_binary_weights_are_the_region_maps_to_the_bit(eng, dtype, D, r):
    """Two images with r tokens of byte 255 at different positions inside N = 256 and byte 0 elsewhere; the rows of weight 0 hold NaN
    in the soft call: they are never read."""
    N, H = 256, 2
    ts = _feats(2, 100 + r + D, dtype, N, H, D)
    w = _weights(N, [r, r], 7 * r + D, 255, 255)
    assert not torch.equal(w[0], w[1]) and sorted(set(w.flatten().tolist())) == [0, 255]
    ia, ib = _idx(0, 1, 0), _idx(1, 0, 0)
    for sim in SIMS:
        want = eng.pair_score_maps_regions(*ts, w != 0, ia, ib, H, sim, return_status=True)
        got = eng.pair_score_maps_weights(*_poison(ts, w), w, ia, ib, H, sim, return_status=True, return_sums=True)
        for name, a, b in zip(("score", "local", "contrib", "status"), got, want):
            assert torch.equal(a, b), (sim, name)
        assert got[4].tolist() == [255 * r, 255 * r]


# ---- 2. general bytes against float64 ------------------------------------------------------------------------------------------------
def _check64(eng, ts, w, pairs, H, sim, dtype, peaked, label):
    """the checks of one float64 case; prints and returns the largest (score err / gate, local err / gate)"""
    N = ts[0].shape[2]
    ia, ib = _idx(*(a for a, _ in pairs)), _idx(*(b for _, b in pairs))
    score, local, contrib, st = eng.pair_score_maps_weights(*_poison(ts, w), w, ia, ib, H, sim, return_status=True)
    assert score.shape == (len(pairs),) and local.shape == contrib.shape == (len(pairs), 2, N)
    assert st.tolist() == [0] * len(pairs)
    want = soft_maps64(*ts, w, ia.cpu(), ib.cpu(), H, sim, dtype)
    soft = eng.pair_score_weights(*ts, w, ia, ib, H, sim)
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
        ss = float(soft[p])
        if abs(gs - ss) > 1e-6 * max(1.0, abs(ss)):
            msgs.append(f"pair_score_weights pair {pairs[p]}: {gs} vs {ss}")
        for d in range(2):
            off = w[pairs[p][d]] == 0
            zeros = torch.zeros(int(off.sum()), device="cuda")
            for name, m in (("local", local), ("contrib", contrib)):         # +0.0f exactly: the bits, not the value
                if not torch.equal(m[p, d][off].view(torch.int32), zeros.view(torch.int32)):
                    msgs.append(f"{name} at the weight-0 tokens of pair {pairs[p]} direction {d} is not +0.0")
    print(f"{label} {str(dtype)[6:]} {sim} peaked={peaked}: score err/gate {worst_s:.3f} local err/gate {worst_l:.3f}")
    assert not msgs, msgs
    return worst_s, worst_l


@pytest.mark.parametrize("N,H,D", [(256, 8, 160), (256, 4, 40), (196, 8, 72), (64, 4, 32)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sim", SIMS)
@pytest.mark.parametrize("peaked", [False, True])
def test_general_bytes_match_float64(eng, dtype, N, H, D, sim, peaked):
    """Four images with unequal numbers of listed tokens, bytes uniform in 1 .. 255; the pairs chain them and (1, 1) is an image with
    itself.  The values carry a channel mean for tests/test_gpu_soft_regions.py's reason."""
    ts = _feats(4, 41 + N + D, dtype, N, H, D, logit_scale=4.0 if peaked else 1.0, channel_mean=1.0)
    sizes = _sizes(N)
    assert len(set(sizes)) == 4 and max(sizes) <= N
    w = _weights(N, sizes, N + D)
    _check64(eng, ts, w, [(0, 1), (1, 2), (2, 3), (3, 0), (1, 1)], H, sim, dtype, peaked, f"N={N} H={H} D={D}")


@pytest.mark.parametrize("sim", SIMS)
def test_several_query_tiles_and_early_leaving_workgroups(eng, sim):
    """bf16 (1024, 8, 80) with 700 and 130 listed tokens: six query tiles of one image, two of the other, workgroups past the counts
    leave early."""
    N, H, D = 1024, 8, 80
    ts = _feats(2, 77, torch.bfloat16, N, H, D, channel_mean=1.0)
    w = _weights(N, [700, 130], 5)
    _check64(eng, ts, w, [(0, 1)], H, sim, torch.bfloat16, False, "N=1024 700/130")


# ---- 3. weights are multiplicities -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,D", [(2, 160), (4, 40)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_weight_is_a_multiplicity(eng, dtype, H, D):
    """tests/test_gpu_soft_regions.py::test_a_weight_is_a_multiplicity's two calls: X with 128 tokens of even bytes 2c against X' with
    every token twice (identical rows) at byte c; Y the same image in both.  The scores agree within twice the gate, and a doubled
    token's two contribs are equal to the bit (identical rows, identical weights) and sum to the single token's contrib within twice
    the score gate times that contrib's share (absolute: 2 gate, the contribs being terms of the score)."""
    n1 = 128
    ts = _feats(2, 57 + D, dtype, n1, H, D)
    g = torch.Generator().manual_seed(5)
    cx = torch.randint(1, 128, (n1,), generator=g)
    cx[::9] = 0
    wy = torch.randint(0, 256, (n1,), generator=g)
    small_w = torch.stack([2 * cx, wy]).to(torch.uint8).cuda()
    twice = tuple(torch.stack([t[0].repeat_interleave(2, 1), torch.cat([t[1], torch.full_like(t[1], float("nan"))], 1)]).contiguous()
                  for t in ts)
    twice_w = torch.stack([cx.repeat_interleave(2), torch.cat([wy, torch.zeros(n1, dtype=wy.dtype)])]).to(torch.uint8).cuda()
    ia, ib = _idx(0), _idx(1)
    for sim in SIMS:
        a = eng.pair_score_maps_weights(*ts, small_w, ia, ib, H, sim, return_status=True)
        b = eng.pair_score_maps_weights(*twice, twice_w, ia, ib, H, sim, return_status=True)
        assert a[3].tolist() == b[3].tolist() == [0]
        gate = 2 * _gate(dtype, False, sim)
        e = _score_err(float(a[0][0]), float(b[0][0]), sim, dtype)
        print(f"multiplicity D={D} {dtype} {sim}: {float(a[0][0]):.8f} vs {float(b[0][0]):.8f} err {e:.3e} gate {gate:.1e}")
        assert e <= gate
        halves = b[2][0, 0].view(n1, 2)                          # direction 0: X' 's tokens, two per token of X
        assert torch.equal(halves[:, 0], halves[:, 1])
        one = a[2][0, 0].double()
        scale = max(abs(float(a[0][0])), 1e-6) if (sim == "mse" or dtype == torch.float32) else 1.0
        assert (halves.double().sum(1) - one).abs().sum().item() <= gate * scale      # (the contribs of a direction sum to <= 2 |score|)
        assert torch.equal(b[1][0, 0].view(n1, 2)[:, 0] == 0, cx.cuda() == 0)          # local: zero exactly where X has no weight


# ---- 4. bit-level invariants -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float16, 144, 2, 72), (torch.float32, 256, 4, 40)])
def test_batch_repeat_swap_and_optional_outputs(eng, dtype, N, H, D):
    from diffsim_amd import _lib
    from diffsim_amd.engine import _TORCH2DSIM
    n = 6
    ts = _feats(n, 71, dtype, N, H, D)
    w = _weights(N, [N, 129 if N == 256 else 100, 64, 1, 33, 100], 9)
    g = torch.Generator().manual_seed(3)
    ia = torch.randint(0, n, (16,), generator=g, dtype=torch.int32).cuda()
    ib = torch.randint(0, n, (16,), generator=g, dtype=torch.int32).cuda()
    L = _lib.lib()
    need = int(L.dsim_pair_score_maps_weights_workspace_bytes(n, 16, B, H, N, D))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    for sim in SIMS:
        r1 = eng.pair_score_maps_weights(*ts, w, ia, ib, H, sim)
        assert torch.isfinite(r1[0]).all()
        assert all(torch.equal(a, b) for a, b in zip(r1, eng.pair_score_maps_weights(*ts, w, ia, ib, H, sim)))      # repeat calls
        for p in (0, 7, 15):                                                                     # a pair alone == inside the batch
            one = eng.pair_score_maps_weights(*ts, w, ia[p:p + 1].clone(), ib[p:p + 1].clone(), H, sim)
            assert all(torch.equal(a[0], b[p]) for a, b in zip(one, r1)), (sim, p)
        sw = eng.pair_score_maps_weights(*ts, w, ib, ia, H, sim)                                 # swapping (a, b) swaps the directions
        assert torch.equal(sw[0], r1[0]) and torch.equal(sw[1], r1[1].flip(1)) and torch.equal(sw[2], r1[2].flip(1))
        for want_local, want_contrib in ((False, False), (True, False), (False, True)):          # local and contrib may be NULL
            score = torch.full((16,), -7.0, device="cuda")
            lo = torch.full((16, 2, N), -7.0, device="cuda") if want_local else None
            co = torch.full((16, 2, N), -7.0, device="cuda") if want_contrib else None
            rc = L.dsim_pair_score_maps_weights(ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), w.data_ptr(), n, ia.data_ptr(),
                                                ib.data_ptr(), 16, B, H, N, D, _TORCH2DSIM[dtype], 0 if sim == "cosine" else 1,
                                                score.data_ptr(), lo.data_ptr() if want_local else None,
                                                co.data_ptr() if want_contrib else None, None, None, ws.data_ptr(), need, None)
            torch.cuda.synchronize()
            assert rc == 0 and torch.equal(score, r1[0])
            assert lo is None or torch.equal(lo, r1[1])
            assert co is None or torch.equal(co, r1[2])


# ---- 5. an image without weight, non-finite features ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float32, 144, 2, 72), (torch.float16, 64, 4, 32)])
def test_an_image_without_weight_is_reported_and_leaves_the_others(eng, dtype, N, H, D):
    ts = _feats(4, 81, dtype, N, H, D)
    w = _weights(N, [N // 2, 40, 17, N], 4)
    ia, ib = _idx(0, 1, 2, 3, 2), _idx(1, 2, 3, 0, 2)
    for sim in SIMS:
        clean = eng.pair_score_maps_weights(*ts, w, ia, ib, H, sim, return_status=True)
        assert clean[3].tolist() == [0] * 5
        w2 = w.clone()
        w2[2] = 0
        score, local, contrib, st, sums = eng.pair_score_maps_weights(*ts, w2, ia, ib, H, sim, return_status=True, return_sums=True)
        assert st.tolist() == [0, 2, 2, 0, 2] and sums.tolist() == w2.long().sum(1).tolist() and sums[2].item() == 0
        assert torch.isnan(score[[1, 2, 4]]).all()
        assert not local[[1, 2, 4]].any() and not contrib[[1, 2, 4]].any()
        for got, want in zip((score, local, contrib), clean):
            assert torch.equal(got[[0, 3]], want[[0, 3]])


@pytest.mark.parametrize("dtype,N,H,D", [(torch.float16, 256, 8, 160), (torch.float32, 144, 2, 72)])
def test_a_nan_feature_flags_exactly_its_pairs(eng, dtype, N, H, D):
    ts = _feats(4, 9, dtype, N, H, D)
    w = _weights(N, [N // 2, 40, 90, 64], 6)
    ia, ib = _idx(0, 1, 2), _idx(1, 2, 3)
    clean = eng.pair_score_maps_weights(*ts, w, ia, ib, H, "cosine", return_status=True)
    assert clean[3].tolist() == [0, 0, 0]
    k2 = ts[1].clone()
    k2[3, 1, int(torch.nonzero(w[3])[5]), 5] = float("nan")          # a row of image 3 that has weight
    got = eng.pair_score_maps_weights(ts[0], k2, ts[2], w, ia, ib, H, "cosine", return_status=True)
    assert got[3].tolist() == [0, 0, 1]
    for a, b in zip(got[:3], clean[:3]):
        assert torch.equal(a[:2], b[:2])


# ---- 6. through the scorer and the command line ---------------------------------------------------------------------------------------------
def test_sd15_tiny_soft_maps_and_alignments_from_files(eng, tmp_path):
    """The scorer's soft_region_similarity_maps / soft_region_alignment on image and gray mask files: the engine calls on the same
    features and weights, the score soft_region_score's, .weights the masks' area averages and .mask weights != 0."""
    from diffsim_amd import regions as R
    from diffsim_amd.inputs import path_latents
    from diffsim_amd.scorer import stack_rows
    from tests.test_gpu_soft_regions import _gray_mask_files, _image_files, _sd15_tiny
    ds = _sd15_tiny(torch.float32)
    block, layer = "up_blocks", 0
    tap = ds.tap_of(block, layer)
    heads = ds.engine_at(tap).heads
    imgs, mks = _image_files(tmp_path, 2, 1), _gray_mask_files(tmp_path, 2, 2)
    (latA, latB), nA, nB = path_latents(ds, [(imgs[0], imgs[1])], (0, 1), 128, 2334, 16)
    grid = R.tap_grid(ds, tap, latA.shape[-1])
    q, k, v = ds.tap_features(*stack_rows([latA.cuda(), latB.cuda()], [nA.cuda(), nB.cuda()], 0, 1), ds.bind_prompt("a cat", 1, "pairs"), tap, 600)
    rows = torch.stack([R.as_token_weights(m, grid).flatten() for m in mks]).cuda()
    assert 0 < int(((rows > 0) & (rows < 255)).sum())
    ia, ib = _idx(0), _idx(1)
    for sim in SIMS:
        mp = ds.soft_region_similarity_maps(imgs[0], imgs[1], mks[0], mks[1], 128, "a cat", block, [0], 600, seed=2334, similarity=sim)
        s, lo, co = eng.pair_score_maps_weights(q, k, v, rows, ia, ib, heads, sim)
        assert torch.equal(mp.score, s) and torch.equal(mp.local.flatten(2), lo) and torch.equal(mp.contrib.flatten(2), co)
        assert mp.weights.dtype == torch.uint8 and torch.equal(mp.weights.flatten(2)[0], rows) and torch.equal(mp.mask, mp.weights != 0)
        want = ds.soft_region_score(imgs[0], imgs[1], mks[0], mks[1], 128, "a cat", block, [0], 600, seed=2334, similarity=sim)
        assert abs(float(mp.score[0]) - float(want[0])) <= 1e-6 * max(1.0, abs(float(want[0])))
    al = ds.soft_region_alignment(imgs[0], imgs[1], mks[0], mks[1], 128, "a cat", block, [0], 600, seed=2334)
    m, wt, ex = eng.pair_align_weights(q, k, rows, ia, ib, heads, grid[1])
    assert torch.equal(al.match.flatten(2), m) and torch.equal(al.weight.flatten(2), wt) and torch.equal(al.expect.flatten(2, 3), ex)
    assert torch.equal(al.weights.flatten(2)[0], rows) and bool((al.match[~al.mask] == -1).all()) and bool((al.match[al.mask] >= 0).all())
    # masks of 0 / 255 on the grid: the hard forms' bits
    bw = (torch.rand(2, *grid, generator=torch.Generator().manual_seed(4)) < 0.5)
    bw[:, 0, 0] = True
    hard = ds.region_similarity_maps(imgs[0], imgs[1], bw[0], bw[1], 128, "a cat", block, [0], 600, seed=2334)
    soft = ds.soft_region_similarity_maps(imgs[0], imgs[1], bw[0], bw[1], 128, "a cat", block, [0], 600, seed=2334)
    assert torch.equal(hard.score, soft.score) and torch.equal(hard.local, soft.local) and torch.equal(hard.contrib, soft.contrib)
    assert torch.equal(hard.mask, soft.mask)


def test_cli_writes_soft_region_maps_and_matches(tmp_path, monkeypatch, capsys):
    """--dataset retrieval --soft_masks with mask folders, --save_region_maps and --save_region_matches: one .npz and one .match.npz per
    query whose scores are the ranking file's and whose weights are the mask files' area averages (a gallery image without one: 255)."""
    import os
    import numpy as np
    from diffsim_amd import cli, regions as R
    from tests.test_gpu_soft_regions import _gray_mask_files, _image_files, _sd15_tiny
    ds = _sd15_tiny(torch.float32)
    qdir, gdir, qm, gm, out = (tmp_path / d for d in ("q", "g", "qm", "gm", "out"))
    for d in (qdir, gdir, qm, gm):
        d.mkdir()
    qa, gb = _image_files(qdir, 2, 11), _image_files(gdir, 4, 12)
    qmasks, gmasks = _gray_mask_files(qm, 2, 20), _gray_mask_files(gm, 3, 30) + [None]
    for paths, masks in ((qa, qmasks), (gb, gmasks)):                      # a mask file carries its image's name
        for i, (p, m) in enumerate(zip(paths, masks)):
            if m is not None:
                masks[i] = os.path.join(os.path.dirname(m), os.path.basename(p))
                os.rename(m, masks[i])
    gmask_of = dict(zip(gb, gmasks))
    monkeypatch.setattr(cli, "build_scorer", lambda args: ds)
    args = cli.arg_parse(["--dataset", "retrieval", "--query_path", str(qdir), "--image_path", str(gdir), "--out_path", str(out),
                          "--image_size", "128", "--target_block", "up_blocks", "--target_layer", "0", "--target_step", "600",
                          "--similarity", "cosine", "--topk", "3", "--query_mask_path", str(qm), "--gallery_mask_path", str(gm),
                          "--soft_masks", "--save_region_maps", "--save_region_matches"])
    assert cli.run(args) == 0
    text = capsys.readouterr().out
    assert "Soft score matrix" in text and "Soft region maps" in text and "Soft region alignments" in text
    for i, name in enumerate(("img11_0", "img11_1")):
        rank = [line.split() for line in open(out / f"{name}.txt").read().splitlines()]
        z, zm = np.load(out / f"{name}.npz"), np.load(out / f"{name}.match.npz")
        assert list(z["gallery"]) == [r[0] for r in rank] == list(zm["gallery"])
        for s, r in zip(z["score"].tolist(), rank):
            assert abs(s - float(r[1])) <= 1e-6 * max(1.0, abs(float(r[1]))), (name, s, r)
        grid = z["local"].shape[2:]
        assert z["weights"].shape == z["local"].shape == (3, 2, *grid) and z["weights"].dtype == np.uint8
        assert np.array_equal(z["weights"], zm["weights"]) and np.array_equal(z["mask"], z["weights"] != 0)
        for j, gpath in enumerate(z["gallery"]):
            assert np.array_equal(z["weights"][j, 0], R.as_token_weights(qmasks[i], grid).numpy())
            assert np.array_equal(z["weights"][j, 1], R.as_token_weights(gmask_of[str(gpath)], grid).numpy())
        assert ((z["weights"] > 0) & (z["weights"] < 255)).any()
        assert not z["local"][~z["mask"]].any() and (zm["match"][~zm["mask"]] == -1).all() and (zm["match"][zm["mask"]] >= 0).all()
        assert np.allclose(0.5 * z["contrib"].astype(np.float64).sum((1, 2, 3)), z["score"], rtol=0, atol=1e-6)
