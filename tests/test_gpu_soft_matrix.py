"""Soft score matrices (dsim_score_matrix_weights / engine.score_matrix_weights / retrieval's soft=True): every image of set A under
its token weights against every image of set B under its own.  A cell is the soft region score of its pair, so it is checked to the
bit against engine.pair_score_weights over the same cells, against engine.score_matrix_regions where every byte is 0 or 255,
against engine.score_matrix where every byte is 255, against the float64 restatement tests/_soft64.py, and for what the header
promises: rows of weight 0 are never read, an image without weight is reported in its row or column alone, a cell does not depend
on its neighbours or its set.

Features, weights and gates are tests/test_gpu_soft_regions.py's (_feats, _weights, _poison, _sizes, _gate, _score_err), imported.

Recorded, not used -- the first MI355X run's largest err / gate against float64 per dtype (test_general_weights_match_float64, all
shapes, both similarities, normal and peaked):

    dtype      largest err / gate
    float32    0.008
    bfloat16   0.007
    float16    0.007
"""
import os

import pytest
import torch

from tests._soft64 import Soft64
from tests.test_gpu_soft_regions import (B, DTYPES, SIMS, _feats, _gate, _gray_mask_files, _image_files, _poison, _score_err, _sd15_tiny,
                                         _sizes, _weights)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


def _split(ts, w, n_a):
    """the first n_a images as set A, the rest as set B: (fa, fb, weights_a, weights_b), each contiguous"""
    return (tuple(t[:n_a].contiguous() for t in ts), tuple(t[n_a:].contiguous() for t in ts), w[:n_a].contiguous(), w[n_a:].contiguous())


def _cells(n_a, n_b):
    """the pair indices of the n_a x n_b cells over the concatenated sets, row-major"""
    ia = torch.arange(n_a, dtype=torch.int32).repeat_interleave(n_b).cuda()
    ib = (n_a + torch.arange(n_b, dtype=torch.int32)).repeat(n_a).cuda()
    return ia, ib


# ---- 1. the soft pair tail over the same cells, to the bit ----------------------------------------------------------------------------
# seven different numbers of listed tokens per shape (three query images, four gallery images) around the 32-row, 64-key and
# 128-query boundaries; every image of a matrix is a query in one direction and the keys in the other
COUNTS = {(256, 2, 160): [1, 32, 63, 65, 128, 255, 256],
          (256, 4, 40): [129, 256, 31, 64, 200, 33, 127],
          (144, 2, 72): [144, 1, 32, 63, 64, 129, 33],
          (200, 2, 64): [31, 33, 64, 127, 129, 200, 1],
          (64, 4, 32): [64, 1, 31, 32, 33, 63, 17]}


@pytest.mark.parametrize("N,H,D", list(COUNTS))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sim", SIMS)
def test_equals_the_soft_pair_tail(eng, dtype, N, H, D, sim):
    """Bytes uniform in 1 .. 255 at the listed tokens; the rows of weight 0 hold NaN in the matrix call: they are never read."""
    counts = COUNTS[(N, H, D)]
    assert len(set(counts)) == 7 and max(counts) <= N
    ts = _feats(7, 100 + N + D, dtype, N, H, D)
    w = _weights(N, counts, N + D)
    assert (w != 0).sum(1).tolist() == counts and len(set(w.flatten().tolist())) > 100
    fa, fb, wa, wb = _split(_poison(ts, w), w, 3)
    got, st, sums = eng.score_matrix_weights(fa, fb, wa, wb, H, sim, return_status=True, return_sums=True)
    want, wst, wsums = eng.pair_score_weights(*ts, w, *_cells(3, 4), H, sim, return_status=True, return_sums=True)
    assert torch.equal(sums, wsums) and sums.tolist() == w.long().sum(1).tolist()
    assert torch.equal(got, want.view(3, 4)), (got, want)
    assert torch.equal(st, wst.view(3, 4)) and not st.any()


# ---- 2. bytes 0 / 255: the region matrix; every byte 255: the score matrix ------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 63, 64, 65, 127, 128, 129, 255])
@pytest.mark.parametrize("H,D", [(2, 160), (4, 40)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_binary_weights_are_the_region_matrix_to_the_bit(eng, dtype, H, D, r):
    """Four images with r tokens of byte 255 at different positions inside N = 256 and byte 0 elsewhere (NaN rows there)."""
    N = 256
    ts = _feats(4, 100 + r + D, dtype, N, H, D)
    w = _weights(N, [r] * 4, 7 * r + D, 255, 255)
    assert sorted(set(w.flatten().tolist())) == [0, 255] and not torch.equal(w[0], w[2])
    fa, fb, wa, wb = _split(ts, w, 2)
    ba, bb, _, _ = _split(_poison(ts, w), w, 2)
    for sim in SIMS:
        want, wst, cnt = eng.score_matrix_regions(fa, fb, wa != 0, wb != 0, H, sim, return_status=True, return_counts=True)
        got, st, sums = eng.score_matrix_weights(ba, bb, wa, wb, H, sim, return_status=True, return_sums=True)
        assert torch.equal(got, want), (sim, got, want)
        assert torch.equal(st, wst) and not st.any()
        assert sums.tolist() == (255 * cnt).tolist() == [255 * r] * 4


@pytest.mark.parametrize("dtype,N,H,D", [(torch.float32, 256, 2, 160), (torch.float32, 144, 2, 72), (torch.bfloat16, 256, 4, 40),
                                         (torch.float16, 256, 4, 40)])
def test_full_weights_are_the_score_matrix(eng, dtype, N, H, D):
    """(wherever score_matrix is the tiled kernel)"""
    ts = _feats(5, 21 + N + D, dtype, N, H, D)
    fa, fb, wa, wb = _split(ts, torch.full((5, N), 255, dtype=torch.uint8, device="cuda"), 2)
    for sim in SIMS:
        got, st = eng.score_matrix_weights(fa, fb, wa, wb, H, sim, return_status=True)
        want, wst = eng.score_matrix(fa, fb, H, sim, return_status=True)
        assert torch.equal(got, want) and torch.equal(st, wst), (sim, got, want)


# ---- 3. general weights against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,D", [(256, 8, 160), (256, 4, 40), (144, 2, 72), (64, 4, 32)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("peaked", [False, True])
def test_general_weights_match_float64(eng, dtype, N, H, D, peaked):
    """tests/test_gpu_soft_regions.py::test_general_weights_match_float64's images, weights and gates, as a 2 x 2 matrix: set A holds
    the largest and the third numbers of listed tokens, set B the others."""
    ts = _feats(4, 41 + N + D, dtype, N, H, D, logit_scale=4.0 if peaked else 1.0, channel_mean=1.0)
    sizes = _sizes(N)
    w = _weights(N, sizes, N + D)
    order = [0, 2, 1, 3]
    ts, w = tuple(t[order].contiguous() for t in ts), w[order].contiguous()
    fa, fb, wa, wb = _split(_poison(ts, w), w, 2)
    ref = Soft64(*ts, w, H, dtype)
    worst = 0.0
    for sim in SIMS:
        got, st = eng.score_matrix_weights(fa, fb, wa, wb, H, sim, return_status=True)
        assert not st.any()
        gate = _gate(dtype, peaked, sim)
        errs = {(i, j): _score_err(float(got[i, j]), ref.pair(i, 2 + j, sim), sim, dtype) for i in range(2) for j in range(2)}
        print(f"{dtype} N={N} H={H} D={D} {sim} peaked={peaked}: errs {' '.join(f'{e:.3e}' for e in errs.values())} gate {gate:.1e}")
        for c, e in errs.items():
            assert e <= gate, (sim, c, float(got[c]), e)
        worst = max(worst, max(errs.values()) / gate)
    print(f"largest err / gate {dtype}: {worst:.3f}")


# ---- 4. an image without weight ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float32, 144, 2, 72), (torch.float16, 64, 4, 32)])
def test_an_image_without_weight_marks_its_row_or_column_alone(eng, dtype, N, H, D):
    ts = _feats(7, 81, dtype, N, H, D)
    counts = [N // 2, 0, 40, 17, N, 0, 33]                     # query 1 and gallery image 2 (index 5) have no weight
    w = _weights(N, counts, 4)
    fa, fb, wa, wb = _split(ts, w, 3)
    keep_a, keep_b = torch.tensor([0, 2]).cuda(), torch.tensor([0, 1, 3]).cuda()
    for sim in SIMS:
        got, st, sums = eng.score_matrix_weights(fa, fb, wa, wb, H, sim, return_status=True, return_sums=True)
        assert sums.tolist() == w.long().sum(1).tolist() and sums[1].item() == sums[5].item() == 0
        want_st = torch.zeros(3, 4, dtype=torch.int32)
        want_st[1, :] = 2
        want_st[:, 2] = 2
        assert torch.equal(st.cpu(), want_st)
        assert torch.isnan(got[1, :]).all() and torch.isnan(got[:, 2]).all()
        ga, gb = tuple(t[keep_a].contiguous() for t in fa), tuple(t[keep_b].contiguous() for t in fb)
        clean, cst = eng.score_matrix_weights(ga, gb, wa[keep_a].contiguous(), wb[keep_b].contiguous(), H, sim, return_status=True)
        assert not cst.any() and torch.isfinite(clean).all()
        assert torch.equal(got[keep_a][:, keep_b], clean), (sim, got, clean)
    none = torch.zeros_like(w)                                  # every image without weight: the call itself is fine
    got, st = eng.score_matrix_weights(fa, fb, none[:3].contiguous(), none[3:].contiguous(), H, "cosine", return_status=True)
    assert torch.isnan(got).all() and (st == 2).all()


# ---- 5. independence and symmetry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float16, 144, 2, 72), (torch.float32, 256, 4, 40)])
def test_alone_repeat_streams_transpose_and_self(eng, dtype, N, H, D):
    ts = _feats(6, 71, dtype, N, H, D)
    w = _weights(N, [N, 129, 64, 1, 33, 100], 9)
    fa, fb, wa, wb = _split(ts, w, 2)
    for sim in SIMS:
        r1 = eng.score_matrix_weights(fa, fb, wa, wb, H, sim)
        assert torch.isfinite(r1).all()
        assert torch.equal(r1, eng.score_matrix_weights(fa, fb, wa, wb, H, sim))                          # a repeat call
        for i in range(2):                                                                                  # a cell alone
            for j in range(4):
                one = eng.score_matrix_weights(tuple(t[i:i + 1] for t in fa), tuple(t[j:j + 1] for t in fb), wa[i:i + 1], wb[j:j + 1], H, sim)
                assert torch.equal(one[0, 0], r1[i, j]), (sim, i, j)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]                                                # two streams
        torch.cuda.synchronize()
        res = []
        for s in streams:
            with torch.cuda.stream(s):
                res.append(eng.score_matrix_weights(fa, fb, wa, wb, H, sim))
        torch.cuda.synchronize()
        assert torch.equal(res[0], r1) and torch.equal(res[1], r1)
        assert torch.equal(eng.score_matrix_weights(fb, fa, wb, wa, H, sim).T, r1)                        # the sets swapped
        own = eng.score_matrix_weights(ts, ts, w, w, H, sim)                                              # an image in both sets
        assert own.diagonal().tolist() == [1.0 if sim == "cosine" else 0.0] * 6, (sim, own.diagonal())
        assert torch.equal(own, own.T)
        assert torch.equal(own[:2, 2:], r1)                                                                 # ... and a cell in a bigger matrix


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(eng):
    """DSIM_ERR_WORKSPACE for a workspace one byte short of what the launcher needs (the query's answer less its 256 bytes of
    alignment slack; the pointer here is aligned), DSIM_ERR_INVALID with a workspace query of 0 for n_a = 0, a head dim outside the
    set and a bad dtype; the output keeps its bytes in every case."""
    from diffsim_amd import _lib
    L = _lib.lib()
    OK, INVALID, WORKSPACE = 0, -1, -3                          # include/diffsim_amd.h: DSIM_OK, DSIM_ERR_INVALID, DSIM_ERR_WORKSPACE
    N, H, D = 64, 4, 32
    ts = _feats(3, 91, torch.bfloat16, N, H, D)
    w = _weights(N, [N, 20, 7], 1)
    query = L.dsim_score_matrix_weights_workspace_bytes
    need = int(query(1, 2, B, H, N, D, _lib.DSIM_BF16))
    assert need > 256
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    out = torch.full((2,), -7.0, device="cuda")
    sums = torch.full((3,), -7, dtype=torch.int32, device="cuda")

    def call(n_a=1, D_=D, dtype=_lib.DSIM_BF16, sim=0, wsb=need):
        rc = L.dsim_score_matrix_weights(ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), w.data_ptr(), n_a,
                                         ts[0][1:].data_ptr(), ts[1][1:].data_ptr(), ts[2][1:].data_ptr(), w[1:].data_ptr(), 2, B, H, N, D_,
                                         dtype, sim, out.data_ptr(), None, sums.data_ptr(), ws.data_ptr(), wsb, None)
        torch.cuda.synchronize()
        return rc
    assert call(wsb=need - 257) == WORKSPACE
    assert call(n_a=0) == INVALID and query(0, 2, B, H, N, D, _lib.DSIM_BF16) == 0
    assert call(D_=24) == INVALID and query(1, 2, B, H, N, 24, _lib.DSIM_BF16) == 0
    assert call(dtype=9) == INVALID and query(1, 2, B, H, N, D, 9) == 0
    assert call(sim=2) == INVALID
    assert out.tolist() == [-7.0, -7.0] and sums.tolist() == [-7, -7, -7]
    assert call(wsb=need - 256) == OK                # the same call with the workspace it needs
    want = eng.score_matrix_weights(tuple(t[:1] for t in ts), tuple(t[1:] for t in ts), w[:1], w[1:], H)
    assert torch.equal(out, want[0]) and sums.tolist() == w.long().sum(1).tolist()


# ---- 7. through the scorer and the command line -------------------------------------------------------------------------------------------
def _gray_weights(n, grid, seed):
    """(n, h, w) uint8: a third of the tokens 0, a third 255, the rest any byte; token (0, 0) on"""
    g = torch.Generator().manual_seed(seed)
    kind = torch.randint(0, 3, (n, *grid), generator=g)
    w = torch.where(kind == 0, 0, torch.where(kind == 1, 255, torch.randint(1, 255, (n, *grid), generator=g))).to(torch.uint8)
    w[:, 0, 0] = 255
    return w


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sd15_tiny_latent_matrix_equals_the_soft_pairs(dtype, tmp_path):
    from diffsim_amd import regions as R
    from diffsim_amd.inputs import path_latents
    from diffsim_amd.retrieval import score_latent_matrix
    ds = _sd15_tiny(dtype)
    qa, gb = _image_files(tmp_path, 3, 1), _image_files(tmp_path, 3, 2)
    (latA,), nA, _ = path_latents(ds, [(p,) for p in qa], (0,), 128, 2334, 16)
    (latB,), _, nB = path_latents(ds, [(p,) for p in gb], (1,), 128, 2334, 16)
    block, layer = "up_blocks", 0
    grid = R.tap_grid(ds, ds.tap_of(block, layer), latA.shape[-1])
    wA, wB = _gray_weights(3, grid, 5), _gray_weights(3, grid, 6)
    full = torch.full((3, *grid), 255, dtype=torch.uint8)
    for sim in SIMS:
        m = score_latent_matrix(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, masks_a=wA, masks_b=wB, soft=True)
        cells = R.score_latent_pair_weights(ds, latA.repeat_interleave(3, 0), latB.repeat(3, 1, 1, 1), nA, nB, wA.repeat_interleave(3, 0),
                                            wB.repeat(3, 1, 1), "a cat", block, layer, 600, sim).view(3, 3)
        assert torch.equal(m, cells), (sim, m, cells)                                        # cell by cell
        two = score_latent_matrix(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, batch=2, masks_a=wA, masks_b=wB, soft=True)
        assert torch.equal(two, m)                                                           # two gallery chunks
        assert not torch.equal(m, score_latent_matrix(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, masks_a=wA != 0, masks_b=wB != 0))
        only_a = score_latent_matrix(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, masks_a=wA, soft=True)
        assert torch.equal(only_a, score_latent_matrix(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, masks_a=wA, masks_b=full,
                                                       soft=True))
        hard = score_latent_matrix(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, masks_a=wA >= 128, masks_b=wB >= 128)
        assert torch.equal(hard, score_latent_matrix(ds, latA, latB, nA, nB, "a cat", block, layer, 600, sim, masks_a=wA >= 128,
                                                     masks_b=wB >= 128, soft=True))         # bool masks: the region matrix's bits


def test_cli_ranks_with_soft_masks(tmp_path, monkeypatch, capsys):
    """--dataset retrieval --soft_masks --query_mask_path --gallery_mask_path on generated images and gray mask folders (one gallery
    image has no mask file): the ranking files are retrieval.topk of score_path_matrix(soft=True) with the same masks."""
    from diffsim_amd import cli, retrieval
    ds = _sd15_tiny(torch.float32)
    qdir, gdir, qm, gm, out = (tmp_path / d for d in ("q", "g", "qm", "gm", "out"))
    for d in (qdir, gdir, qm, gm):
        d.mkdir()
    qa, gb = _image_files(qdir, 2, 11), _image_files(gdir, 4, 12)
    qmasks = _gray_mask_files(qm, 2, 20)
    gmasks = _gray_mask_files(gm, 3, 30) + [None]
    for paths, masks in ((qa, qmasks), (gb, gmasks)):                      # a mask file carries its image's name
        for i, (p, m) in enumerate(zip(paths, masks)):
            if m is not None:
                masks[i] = os.path.join(os.path.dirname(m), os.path.basename(p))
                os.rename(m, masks[i])
    monkeypatch.setattr(cli, "build_scorer", lambda args: ds)
    args = cli.arg_parse(["--dataset", "retrieval", "--query_path", str(qdir), "--image_path", str(gdir), "--out_path", str(out),
                          "--image_size", "128", "--target_block", "up_blocks", "--target_layer", "0", "--target_step", "600",
                          "--similarity", "cosine", "--topk", "3", "--query_mask_path", str(qm), "--gallery_mask_path", str(gm),
                          "--soft_masks"])
    assert cli.run(args) == 0
    said = capsys.readouterr().out
    assert "Soft score matrix" in said and "1 image(s) without a mask file" in said
    assert "Mean query token weight" in said and "Mean gallery token weight" in said
    m = retrieval.score_path_matrix(ds, qa, gb, 128, args.prompt, "up_blocks", 0, 600, args.seed, "cosine", masks_a=qmasks, masks_b=gmasks,
                                    soft=True)
    assert not torch.equal(m, retrieval.score_path_matrix(ds, qa, gb, 128, args.prompt, "up_blocks", 0, 600, args.seed, "cosine",
                                                          masks_a=qmasks, masks_b=gmasks))
    vals, idx = retrieval.topk(m, 3, "cosine")
    for i, name in enumerate(("img11_0", "img11_1")):
        rank = [l.split() for l in open(out / f"{name}.txt").read().splitlines()]
        assert [r[0] for r in rank] == [gb[j] for j in idx[i].tolist()]
        assert [float(r[1]) for r in rank] == [float(f"{v:.8g}") for v in vals[i].tolist()]
