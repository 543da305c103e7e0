"""Region maps and region alignments, host side (no GPU): the C ABI's four entry points and their refusals, the command line's
--save_region_maps / --save_region_matches, the mask plumbing of maps.py and align.py on a CPU stand-in, the containers' and the
writers' optional masks, and the float64 restatement tests/_regionmap64.py (the yardstick of tests/test_gpu_region_maps.py and
tests/test_gpu_region_align.py) against tests/_region64.py, tests/_tail64.py and tests/_align64.py."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _align64 as A
from tests import _regionmap64 as R64
from tests._region64 import regions64
from tests._tail64 import pairs64
from tests.test_region_matrix_host import _Scorer as _MatrixScorer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"dsim_pair_score_maps_regions": 22, "dsim_pair_align_regions": 22}


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    assert re.search(r"#define\s+DSIM_ABI_VERSION\s+7\b", hdr)             # additive: the version stays
    from diffsim_amd import _lib
    assert _lib.ABI_VERSION == 7
    for name, nargs in ENTRIES.items():
        assert re.search(rf"size_t\s+{name}_workspace_bytes\s*\(\s*int n_feat,\s*int n_pairs,\s*int B,\s*int H,\s*int N,\s*int D\)", hdr), name
        assert len(_lib.SYMBOLS[f"{name}_workspace_bytes"][1]) == 6
        assert len(_lib.SYMBOLS[name][1]) == nargs
        decl = re.search(rf"int\s+{name}\s*\(([^;]*)\)\s*;", hdr).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == nargs, name
    L = _lib.lib()
    assert L.dsim_version() == 7 and all(hasattr(L, n) and hasattr(L, n + "_workspace_bytes") for n in ENTRIES)


def test_refusals_come_before_any_launch():
    """Every refusal of the two calls is decided on the host before anything is enqueued, so it is checked without a GPU (the
    pointers are never read)."""
    import ctypes
    from diffsim_amd import _lib
    L = _lib.lib()
    B, H, N, D = 2, 4, 64, 32
    up = lambda b: (b + 255) // 256 * 256          # noqa: E731
    maps_ws, align_ws = L.dsim_pair_score_maps_regions_workspace_bytes, L.dsim_pair_align_regions_workspace_bytes
    # lists | counts | the call's own partials / statistics, each 256-byte aligned, and the slack
    assert int(maps_ws(5, 3, B, H, N, D)) == up(5 * N * 4) + up(5 * 4) + up(3 * 2 * 3 * B * H * N * 4) + 256
    assert int(align_ws(5, 3, B, H, N, D)) == up(5 * N * 4) + up(5 * 4) + up(3 * 2 * B * H * N * 8) + 256
    for ws in (maps_ws, align_ws):
        for args in ((0, 3, B, H, N, D), (5, 0, B, H, N, D), (5, 3, B, H, N, 24), (5, 3, B, H, N, 0), (5, 3, B, H, 0, D), (5, 3, 0, H, N, D),
                     (5, 32768, B, H, N, D),                       # 2 n_pairs > 65535
                     (5, 3, 2, 32768, N, D),                       # B H > 65535
                     (1 << 20, 3, B, H, 1 << 11, D)):              # n_feat N >= 2^31
            assert ws(*args) == 0, args
        assert ws(5, 32767, 1, 1, 1, 16) > 0 and ws((1 << 20) - 1, 1, 1, 1, 1 << 11, 16) > 0
    fake = ctypes.c_void_p(0x10000)
    need_m, need_a = int(maps_ws(5, 3, B, H, N, D)), int(align_ws(5, 3, B, H, N, D))

    def maps(n_feat=5, n=3, H=H, N=N, D=D, dtype=_lib.DSIM_BF16, sim=0, ws=need_m, q=fake, mask=fake, score=fake, wsp=fake):
        return L.dsim_strerror(L.dsim_pair_score_maps_regions(q, fake, fake, mask, n_feat, fake, fake, n, B, H, N, D, dtype, sim, score,
                                                              None, None, None, None, wsp, ws, None)).lower()

    def align(n_feat=5, n=3, H=H, N=N, D=D, dtype=_lib.DSIM_BF16, grid_w=8, ws=need_a, q=fake, mask=fake, wsp=fake, attn=None):
        return L.dsim_strerror(L.dsim_pair_align_regions(q, fake, mask, n_feat, fake, fake, n, B, H, N, D, dtype, grid_w, None, None, None,
                                                         attn, None, None, wsp, ws, None)).lower()

    for go, need in ((maps, need_m), (align, need_a)):
        assert b"workspace" in go(ws=need // 2) and b"workspace" in go(ws=need - 257)
        for kw in (dict(dtype=9), dict(dtype=-1), dict(D=24), dict(D=0), dict(n=0), dict(n_feat=0), dict(n_feat=-2), dict(n=32768, ws=1 << 44),
                   dict(H=32768, ws=1 << 44), dict(n_feat=1 << 20, N=1 << 11, ws=1 << 50), dict(q=None), dict(mask=None), dict(wsp=None)):
            assert b"invalid" in go(**kw), (go.__name__, kw)
    for kw in (dict(sim=2), dict(sim=-1), dict(score=None)):
        assert b"invalid" in maps(**kw), kw
    for kw in (dict(grid_w=7), dict(grid_w=0), dict(grid_w=-8)):
        assert b"invalid" in align(**kw), kw
    # an attn of 2 GiB: one pair of 16384 tokens
    big = int(align_ws(2, 1, B, 1, 16384, 16))
    assert big > 0 and b"invalid" in align(n_feat=2, n=1, H=1, N=16384, D=16, grid_w=128, ws=big, attn=fake)


def test_engine_checks_come_before_the_library(monkeypatch):
    from diffsim_amd import _lib, engine
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    N, H, D = 16, 2, 8
    q, k, v = (torch.zeros(3, 2, N, H * D) for _ in range(3))
    ia = torch.zeros(1, dtype=torch.int32)
    mask = torch.ones(3, N, dtype=torch.bool)
    for call in (lambda **kw: engine.pair_score_maps_regions(q, k, v, kw.get("mask", mask), ia, ia, H),
                 lambda **kw: engine.pair_align_regions(q, k, kw.get("mask", mask), ia, ia, H)):
        with pytest.raises(_lib.DsimError, match="not on the GPU"):
            call()


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_the_region_output_flags(capsys):
    from diffsim_amd.cli import arg_parse
    base = ["--dataset", "retrieval", "--image_path", "g", "--query_path", "q", "--out_path", "o"]
    a = arg_parse(base + ["--query_mask_path", "qm", "--save_region_maps"])
    assert a.save_region_maps and not a.save_region_matches and not a.save_maps
    a = arg_parse(base + ["--gallery_mask_path", "gm", "--save_region_matches", "--save_region_maps"])
    assert a.save_region_maps and a.save_region_matches and not a.save_matches
    a = arg_parse(base + ["--query_mask_path", "qm"])
    assert not a.save_region_maps and not a.save_region_matches
    for metric in ("diffsim", "diffsim_xl", "dit"):
        assert arg_parse(base + ["--metric", metric, "--query_mask_path", "qm", "--save_region_maps"]).save_region_maps

    def refused(argv, named):
        with pytest.raises(SystemExit) as e:
            arg_parse(argv)
        assert e.value.code == 2
        msg = capsys.readouterr().err.split("error:")[-1]
        assert named in msg, (argv, msg)

    for flag in ("--save_region_maps", "--save_region_matches"):
        refused(base + [flag], flag)                                              # no mask flag
        for dataset in ("cute", "nights", "sref"):
            refused(["--dataset", dataset, flag], flag)
            refused(["--dataset", dataset, "--mask_path", "m", flag], flag)
        for metric in ("clip_cross", "dino_cross"):
            refused(base + ["--metric", metric, "--query_mask_path", "qm", flag], flag)
        refused(base + ["--query_mask_path", "qm", flag, "--taps", "up_blocks:0"], flag)
        refused(base + ["--query_mask_path", "qm", flag, "--text_attn"], flag)
    # the whole-image flags stay refused with masks, and now point at the region flags
    for flag, new in (("--save_maps", "--save_region_maps"), ("--save_matches", "--save_region_matches")):
        refused(base + ["--query_mask_path", "qm", flag], "--query_mask_path")
        with pytest.raises(SystemExit):
            arg_parse(base + ["--gallery_mask_path", "gm", flag])
        assert new in capsys.readouterr().err.split("error:")[-1]


# ---- the mask plumbing of maps.py and align.py on a CPU stand-in ----------------------------------------------------------------------
class _Scorer(_MatrixScorer):
    """test_region_matrix_host's stand-in plus what Scorer.pair_chunks asks for; pair_chunks itself is the real one"""
    one_tap_bound = False

    def auto_map_pairs(self, eng, n):
        return 2

    def chunk_prompt(self, prompt, i0, i1, per_row):
        return prompt

    from diffsim_amd.scorer import Scorer as _S
    pair_chunks = _S.pair_chunks
    del _S


def _lat(seed, n):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 4, 4, 4, generator=g), torch.randn(n, 4, 4, 4, generator=g), torch.randn(1, 4, 4, 4, generator=g)


def test_pair_map_masks_reach_the_region_call_and_none_changes_nothing(monkeypatch):
    from diffsim_amd import maps as M
    calls = []

    def whole(q, k, v, ia, ib, heads, sim):
        calls.append(("whole", q.shape[0]))
        n, N = ia.numel(), q.shape[2]
        return torch.zeros(n), torch.zeros(n, 2, N), torch.zeros(n, 2, N)

    def regions(q, k, v, mask, ia, ib, heads, sim):
        calls.append(("regions", mask.clone()))
        assert mask.dtype == torch.bool and mask.shape == (q.shape[0], q.shape[2]) and mask.is_contiguous()
        want = R64.region_maps64(q, k, v, mask, ia, ib, heads, sim, torch.float32)
        return (torch.tensor([w[0] for w in want], dtype=torch.float32), torch.stack([w[1] for w in want]).float(),
                torch.stack([w[2] for w in want]).float())

    monkeypatch.setattr(M, "pair_score_maps", whole)
    monkeypatch.setattr(M, "pair_score_maps_regions", regions)
    sc = _Scorer()
    la, lb, nz = _lat(3, 3)
    plain = M.score_latent_pair_maps(sc, la, lb, nz, nz, "p")
    assert [c[0] for c in calls] == ["whole", "whole"] and plain.mask is None           # chunks of 2 pairs, today's path
    calls.clear()
    g = torch.Generator().manual_seed(4)
    mA, mB = torch.rand(3, 4, 4, generator=g) < 0.5, torch.rand(3, 16, generator=g) < 0.5
    mA[:, 0, 0] = mB[:, 0] = True
    mp = M.score_latent_pair_maps(sc, la, lb, nz, nz, "p", maskA=mA, maskB=mB)
    assert [c[0] for c in calls] == ["regions", "regions"]
    # a chunk's mask rows interleave as its images do: A0, B0, A1, B1
    assert torch.equal(calls[0][1], torch.stack([mA[0].flatten(), mB[0], mA[1].flatten(), mB[1]]))
    assert torch.equal(calls[1][1], torch.stack([mA[2].flatten(), mB[2]]))
    assert mp.mask.dtype == torch.bool and mp.mask.shape == (3, 2, 4, 4)
    assert torch.equal(mp.mask[:, 0], mA) and torch.equal(mp.mask[:, 1].flatten(1), mB)
    assert not mp.local[~mp.mask].any() and not mp.contrib[~mp.mask].any()
    assert torch.allclose(0.5 * mp.contrib.double().sum((1, 2, 3)), mp.score.double(), atol=1e-6)
    one = M.score_latent_pair_maps(sc, la, lb, nz, nz, "p", batch_pairs=1, maskA=mA, maskB=mB)
    assert torch.equal(one.score, mp.score) and torch.equal(one.local, mp.local)
    assert torch.equal(mp[1:].mask, mp.mask[1:]) and mp[0].mask.shape == (1, 2, 4, 4)
    calls.clear()
    only_b = M.score_latent_pair_maps(sc, la, lb, nz, nz, "p", maskB=mB)
    assert calls[0][0] == "regions" and calls[0][1][0::2].all() and torch.equal(calls[0][1][1], mB[0])       # the A side whole
    assert only_b.mask[:, 0].all()
    with pytest.raises(ValueError, match="maskA"):
        M.score_latent_pair_maps(sc, la, lb, nz, nz, "p", maskA=mA[:2])
    with pytest.raises(ValueError, match="no token on"):
        M.score_latent_pair_maps(sc, la, lb, nz, nz, "p", maskA=torch.zeros(3, 16))
    with pytest.raises(TypeError):
        M.score_latent_pair_maps(sc, la, lb, nz, nz, "p", "up_blocks", 0, 600, "cosine", None, mA)           # keyword-only
    with pytest.raises(ValueError, match="mask must be bool"):
        M.SimilarityMaps(mp.score, mp.local.flatten(2), mp.contrib.flatten(2), mp.mask.float())


def test_pair_alignment_masks_reach_the_region_call_and_none_changes_nothing(monkeypatch):
    from diffsim_amd import align as AL
    calls = []

    def whole(q, k, ia, ib, heads, grid_w=None):
        calls.append(("whole", grid_w))
        n, N = ia.numel(), q.shape[2]
        return torch.zeros(n, 2, N, dtype=torch.int32), torch.zeros(n, 2, N), torch.zeros(n, 2, N, 2)

    def regions(q, k, mask, ia, ib, heads, grid_w=None):
        calls.append(("regions", mask.clone(), grid_w))
        pairs = list(zip(ia.tolist(), ib.tolist()))
        Pm, _ = R64.region_align64(q, k, mask, pairs, heads, with_bound=False)
        rows = R64.rows_of(mask)
        outs = [[R64.region_outputs64(Pm[p, d], rows[pr[d]], rows[pr[1 - d]], grid_w) for d in range(2)] for p, pr in enumerate(pairs)]
        pick = lambda i: torch.stack([torch.stack([o[i] for o in po]) for po in outs])          # noqa: E731
        return pick(0).to(torch.int32), pick(1).float(), pick(2).float()

    monkeypatch.setattr(AL, "pair_align", whole)
    monkeypatch.setattr(AL, "pair_align_regions", regions)
    sc = _Scorer()
    la, lb, nz = _lat(5, 3)
    plain = AL.score_latent_pair_alignment(sc, la, lb, nz, nz, "p")
    assert calls == [("whole", None), ("whole", None)] and plain.mask is None
    calls.clear()
    g = torch.Generator().manual_seed(6)
    mA, mB = torch.rand(3, 4, 4, generator=g) < 0.5, torch.rand(3, 4, 4, generator=g) < 0.5
    mA[:, 0, 0] = mB[:, 3, 3] = True
    al = AL.score_latent_pair_alignment(sc, la, lb, nz, nz, "p", maskA=mA, maskB=mB)
    assert [c[0] for c in calls] == ["regions", "regions"] and all(c[2] == 4 for c in calls)       # the grid's width
    assert torch.equal(calls[0][1], torch.stack([mA[0], mB[0], mA[1], mB[1]]).flatten(1))
    assert al.mask.shape == (3, 2, 4, 4) and torch.equal(al.mask[:, 0], mA) and torch.equal(al.mask[:, 1], mB)
    off = ~al.mask
    assert (al.match[off] == -1).all() and not al.weight[off].any() and (al.expect[off] == -1).all()
    # an on token's match is an on token of the OTHER image's mask
    for p in range(3):
        for d in range(2):
            m = al.match[p, d][al.mask[p, d]].long()
            assert al.mask[p, 1 - d].flatten()[m].all()
    assert torch.equal(al[2].mask, al.mask[2:3])
    with pytest.raises(ValueError, match="maskB"):
        AL.score_latent_pair_alignment(sc, la, lb, nz, nz, "p", maskB=mB[:, :2])
    with pytest.raises(TypeError):
        AL.score_latent_pair_alignment(sc, la, lb, nz, nz, "p", "up_blocks", 0, 600, None, mA)


def test_writers_store_the_masks(tmp_path):
    from diffsim_amd import align as AL
    from diffsim_amd import maps as M
    n_a, k, N = 2, 2, 16
    g = torch.Generator().manual_seed(7)
    mask = torch.rand(n_a * k, 2, N, generator=g) < 0.5
    mp = M.SimilarityMaps(torch.rand(n_a * k, generator=g), torch.rand(n_a * k, 2, N, generator=g), torch.rand(n_a * k, 2, N, generator=g), mask)
    al = AL.Alignment(torch.zeros(n_a * k, 2, N, dtype=torch.int32), torch.rand(n_a * k, 2, N, generator=g),
                      torch.rand(n_a * k, 2, N, 2, generator=g), mask)
    qs, gs = ["q/a.png", "q/b.png"], ["g/x.png", "g/y.png", "g/z.png"]
    idx = torch.tensor([[2, 0], [1, 2]])
    for i, fn in enumerate(M.write_map_files(str(tmp_path), qs, gs, idx, mp, "q")):
        z = np.load(fn)
        assert z["mask"].dtype == np.bool_ and z["mask"].shape == (k, 2, 4, 4)
        assert np.array_equal(z["mask"], mask[i * k:(i + 1) * k].reshape(k, 2, 4, 4).numpy()) and z["local"].shape == (k, 2, 4, 4)
    for i, fn in enumerate(AL.write_match_files(str(tmp_path), qs, gs, idx, al, "q")):
        z = np.load(fn)
        assert np.array_equal(z["mask"], mask[i * k:(i + 1) * k].reshape(k, 2, 4, 4).numpy()) and z["expect"].shape == (k, 2, 4, 4, 2)
    plain = M.SimilarityMaps(mp.score, mp.local.flatten(2), mp.contrib.flatten(2))
    assert "mask" not in np.load(M.write_map_files(str(tmp_path / "p"), qs, gs, idx, plain, "q")[0]).files


# ---- the float64 yardstick itself -----------------------------------------------------------------------------------------------------
def _inputs(dtype, n=4, N=49, H=2, D=16, seed=5):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(n, 2, N, H * D, generator=g).to(dtype) for _ in range(3))
    mask = torch.rand(n, N, generator=g) < 0.5
    mask[:, 0] = True
    mask[1] = True                      # one full region
    mask[2] = False
    mask[2, 7] = True                   # one single token
    return q, k, v, mask


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("sim", ["cosine", "mse"])
def test_region_maps64_against_region64_and_tail64(dtype, sim):
    N, H = 49, 2
    q, k, v, mask = _inputs(dtype)
    ia, ib = [0, 1, 2, 3, 1], [1, 2, 3, 0, 1]
    got = R64.region_maps64(q, k, v, mask, ia, ib, H, sim, dtype)
    want = regions64(q, k, v, mask, ia, ib, H, sim, dtype)
    for p, ((s, lo, co), w) in enumerate(zip(got, want)):
        assert abs(s - w) <= 1e-12 * max(1.0, abs(w)), (p, s, w)
        assert abs(0.5 * float(co.sum()) - s) <= 1e-12 * max(1.0, abs(s))
        for d, i in enumerate((ia[p], ib[p])):
            assert not lo[d][~mask[i]].any() and not co[d][~mask[i]].any()
    # full masks: tests/_tail64.py exactly
    full = torch.ones(4, N, dtype=torch.uint8) * 255
    for (s, lo, co), (ws, wl, wc) in zip(R64.region_maps64(q, k, v, full, ia, ib, H, sim, dtype), pairs64(q, k, v, ia, ib, H, sim, dtype)):
        assert s == ws and torch.equal(lo, wl) and torch.equal(co, wc)
    # an empty region: NaN and zero maps
    none = mask.clone()
    none[3] = False
    s, lo, co = R64.region_maps64(q, k, v, none, [3], [0], H, sim, dtype)[0]
    assert s != s and not lo.any() and not co.any()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_region_align64_against_align64(dtype):
    N, H, w = 49, 2, 7
    q, k, _, mask = _inputs(dtype)
    pairs = ((0, 1), (2, 0), (3, 3))
    Pm, bound = R64.region_align64(q, k, mask, pairs, H)
    rows = R64.rows_of(mask)
    for p, pr in enumerate(pairs):
        for d in range(2):
            rq, rk = rows[pr[d]], rows[pr[1 - d]]
            inside = torch.zeros(N, N, dtype=torch.bool)
            inside[rq[:, None], rk[None, :]] = True
            assert not Pm[p, d][~inside].any() and not bound[p, d][~inside].any()
            assert (Pm[p, d][inside] > 0).all() and (bound[p, d][inside] > 0).all()
            assert ((Pm[p, d][rq].sum(-1) - 1).abs() <= 1e-12).all()
            # the gathered rows through _align64, and the key count's tiles in the bound (49 keys or fewer: one tile either way)
            pm, bd = A.direction64(q[pr[d]].index_select(1, rq), k[pr[1 - d]].index_select(1, rk), H)
            assert torch.equal(Pm[p, d][rq][:, rk], pm) and torch.equal(bound[p, d][rq][:, rk], bd)
            match, weight, expect = R64.region_outputs64(Pm[p, d], rq, rk, w)
            on = torch.zeros(N, dtype=torch.bool)
            on[rq] = True
            assert (match[~on] == -1).all() and not weight[~on].any() and (expect[~on] == -1).all()
            assert mask[pr[1 - d]][match[on]].all()
            assert torch.equal(weight[on], Pm[p, d][on].max(-1).values)
            assert (expect[on, 0] <= (N - 1) // w).all() and (expect[on, 1] <= w - 1).all() and (expect[on] >= 0).all()
    # full masks: tests/_align64.py exactly, outputs included
    full = torch.ones(4, N, dtype=torch.bool)
    Pf, bf = R64.region_align64(q, k, full, pairs, H)
    Pw, bw = A.align64(q, k, pairs, H)
    assert torch.equal(Pf, Pw) and torch.equal(bf, bw)
    m, wt, e = A.outputs64(Pw[0, 0], w)
    allrows = torch.arange(N)
    gm, gw, ge = R64.region_outputs64(Pf[0, 0], allrows, allrows, w)
    assert torch.equal(gm, m) and torch.equal(gw, wt) and torch.allclose(ge, e, rtol=0, atol=1e-12)


def test_the_bound_counts_the_key_regions_tiles():
    """130 queries over 700 keys: direction64 would count 3 tiles, the kernels walk 11"""
    N, H, D = 1024, 1, 16
    g = torch.Generator().manual_seed(9)
    q, k = (torch.randn(2, 2, N, H * D, generator=g).to(torch.bfloat16) for _ in range(2))
    rq, rk = torch.arange(0, 260, 2), torch.arange(100, 800)
    Pm, bound = R64.region_direction64(q[0], k[1], rq, rk, H)
    pm, bd = A.direction64(q[0].index_select(1, rq), k[1].index_select(1, rk), H)
    extra = bound[rq][:, rk] - bd
    assert torch.allclose(extra, 5 * (11 - 3) * A.U32 * pm, rtol=1e-9, atol=0) and (extra > 0).all()
