"""The three soft forms, host side (no GPU): the C ABI's six entry points, their workspace queries and refusals, the engine's own
checks, tests/_softmap64.py against tests/_regionmap64.py on 0 / 255 bytes and on a hand-written weighted softmax, the command
line's --soft_masks with --dataset retrieval, and retrieval's soft=True on test_region_matrix_host.py's CPU stand-in with
tests/_soft64.py in the library's place."""
import ctypes
import os
import re

import pytest
import torch

from tests._region64 import Region64
from tests._soft64 import Soft64
from tests.test_region_matrix_host import _Scorer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    assert re.search(r"size_t\s+dsim_score_matrix_weights_workspace_bytes\s*\(\s*int n_a,\s*int n_b,\s*int B,\s*int H,\s*int N,\s*int D,"
                     r"\s*int dtype\)", hdr)
    assert re.search(r"#define\s+DSIM_ABI_VERSION\s+7\b", hdr)             # additive: the version stays
    from diffsim_amd import _lib
    assert _lib.ABI_VERSION == 7
    assert len(_lib.SYMBOLS["dsim_score_matrix_weights_workspace_bytes"][1]) == 7
    assert len(_lib.SYMBOLS["dsim_score_matrix_weights"][1]) == 22
    decl = re.search(r"int\s+dsim_score_matrix_weights\s*\(([^;]*)\)\s*;", hdr).group(1)
    args = re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")
    assert len(args) == 22 and "uint8_t* weights_a" in args[3] and "uint8_t* weights_b" in args[8] and "weight_sums" in args[18]
    for name, n_q, n_f in (("dsim_pair_score_maps_weights", 6, 22), ("dsim_pair_align_weights", 6, 22)):
        assert re.search(r"size_t\s+" + name + r"_workspace_bytes\s*\(\s*int n_feat,\s*int n_pairs,\s*int B,\s*int H,\s*int N,\s*int D\)", hdr)
        assert len(_lib.SYMBOLS[name + "_workspace_bytes"][1]) == n_q and len(_lib.SYMBOLS[name][1]) == n_f
        decl = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
        args = re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")
        assert len(args) == n_f and any("uint8_t* weights" in a for a in args) and "weight_sums" in args[n_f - 4]
    L = _lib.lib()
    assert L.dsim_version() == 7
    # the queries: positive at (3, 4, 2, 4, 64, 32), 0 for D = 24, a bad dtype, n_a = 0
    for q in (L.dsim_pair_score_maps_weights_workspace_bytes, L.dsim_pair_align_weights_workspace_bytes):
        assert q(3, 4, 2, 4, 64, 32) > 0
        for bad in ((3, 4, 2, 4, 64, 24), (0, 4, 2, 4, 64, 32), (3, 0, 2, 4, 64, 32), (3, 4, 2, 4, 0, 32), (3, 32768, 2, 4, 64, 32),
                    (1, 1, 1, 1, 8421505, 16)):
            assert q(*bad) == 0, bad
    q = L.dsim_score_matrix_weights_workspace_bytes
    assert q(3, 4, 2, 4, 64, 32, _lib.DSIM_BF16) > 0
    assert q(3, 4, 2, 4, 64, 24, _lib.DSIM_BF16) == 0 and q(3, 4, 2, 4, 64, 32, 9) == 0 and q(0, 4, 2, 4, 64, 32, _lib.DSIM_BF16) == 0


def test_pair_form_refusals_come_before_any_launch():
    from diffsim_amd import _lib
    L = _lib.lib()
    B, H, N, D = 2, 4, 64, 32
    fake = ctypes.c_void_p(0x10000)
    need_m = int(L.dsim_pair_score_maps_weights_workspace_bytes(3, 2, B, H, N, D))
    need_a = int(L.dsim_pair_align_weights_workspace_bytes(3, 2, B, H, N, D))
    # the region forms' workspace, then the biases [n_feat][N up to whole 64-key tiles] and the byte sums
    assert need_m == int(L.dsim_pair_score_maps_regions_workspace_bytes(3, 2, B, H, N, D)) + 3 * 64 * 4 + 256
    assert need_a == int(L.dsim_pair_align_regions_workspace_bytes(3, 2, B, H, N, D)) + 3 * 64 * 4 + 256

    def maps(n_feat=3, n=2, D=D, dtype=_lib.DSIM_BF16, sim=0, ws=need_m, w=fake):
        rc = L.dsim_pair_score_maps_weights(fake, fake, fake, w, n_feat, fake, fake, n, B, H, N, D, dtype, sim, fake, None, None, None, None,
                                            fake, ws, None)
        return L.dsim_strerror(rc).lower()

    def align(n_feat=3, n=2, D=D, dtype=_lib.DSIM_BF16, grid_w=8, ws=need_a, w=fake, attn=None):
        rc = L.dsim_pair_align_weights(fake, fake, w, n_feat, fake, fake, n, B, H, N, D, dtype, grid_w, None, None, None, attn, None, None,
                                       fake, ws, None)
        return L.dsim_strerror(rc).lower()

    assert b"workspace" in maps(ws=need_m - 257) and b"workspace" in align(ws=need_a - 257)
    for kw in (dict(dtype=9), dict(D=24), dict(n=0), dict(n_feat=0), dict(w=None)):
        assert b"invalid" in maps(**kw) and b"invalid" in align(**kw), kw
    assert b"invalid" in maps(sim=2) and b"invalid" in align(grid_w=7) and b"invalid" in align(grid_w=0)


# ---- the float64 restatements themselves ---------------------------------------------------------------------------------------------
def _small(dtype, n=3, N=36, H=2, D=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(n, 2, N, H * D, generator=g).to(dtype) for _ in range(3))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_restatements_equal_the_region_ones_on_binary_bytes(dtype):
    from tests import _regionmap64 as RM
    from tests import _softmap64 as SM
    N, H = 36, 2
    q, k, v = _small(dtype)
    g = torch.Generator().manual_seed(1)
    mask = torch.rand(3, N, generator=g) < 0.5
    mask[:, 0] = True
    mask[2] = False                                              # an image without weight
    w = mask.to(torch.uint8) * 255
    ia, ib = [0, 1, 0, 2], [1, 0, 0, 1]
    for sim in ("cosine", "mse"):
        soft, hard = SM.soft_maps64(q, k, v, w, ia, ib, H, sim, dtype), RM.region_maps64(q, k, v, mask, ia, ib, H, sim, dtype)
        for (ss, sl, sc), (hs, hl, hc) in zip(soft, hard):
            assert (ss == hs or (ss != ss and hs != hs)) and torch.equal(sl, hl) and torch.equal(sc, hc)
    pairs = list(zip(ia, ib))
    sp, sb = SM.soft_align64(q, k, w, pairs, H)
    hp, hb = RM.region_align64(q, k, mask, pairs, H)
    assert torch.equal(sp, hp)
    assert (sb >= hb).all() and torch.equal(sb == 0, hb == 0)                                  # the widened bound, zero at the same entries


def test_a_hand_written_weighted_softmax():
    """One head, one CFG half, D = 1: q = 1 for both queries, keys ln 1, ln 2, ln 3 scaled by sqrt(D) = 1 -- logits 0, ln 2, ln 3 -- at
    bytes 255, 0, 85 (weights 1, 0, 1 / 3): the softmax over the listed keys of (0 + ln 1, ln 3 + ln 1/3) is (1/2, 1/2)."""
    import math
    from tests import _softmap64 as SM
    N = 4
    q = torch.ones(2, 1, N, 1, dtype=torch.float32)
    k = torch.tensor([0.0, math.log(2.0), math.log(3.0), 5.0]).view(1, 1, N, 1).repeat(2, 1, 1, 1)
    w = torch.tensor([[255, 0, 85, 0], [255, 255, 0, 0]], dtype=torch.uint8)
    Pm, bound = SM.soft_align64(q, k, w, [(1, 0)], 1)
    want = torch.zeros(N, N, dtype=torch.float64)
    want[0, 0] = want[0, 2] = want[1, 0] = want[1, 2] = 0.5      # queries: image 1's tokens 0, 1; keys: image 0's tokens 0, 2
    assert torch.allclose(Pm[0, 0], want, rtol=0, atol=1e-7) and (bound[0, 0][want == 0] == 0).all()      # (k is float32: ln 3 is rounded)
    # the mirror: queries image 0's tokens 0, 2 over image 1's keys 0, 1 at weight 1: softmax(0, ln 2) = (1/3, 2/3)
    back = torch.zeros(N, N, dtype=torch.float64)
    back[0, 0] = back[2, 0] = 1.0 / 3
    back[0, 1] = back[2, 1] = 2.0 / 3
    assert torch.allclose(Pm[0, 1], back, rtol=0, atol=1e-7)
    # the maps: v = k, so O_ab of image 1's queries is the mean of (0, ln 3) and contrib carries the query weight
    v = k.clone()
    (score, local, contrib), = SM.soft_maps64(q, k, v, w, [0], [1], 1, "mse", torch.float32)
    # direction 0: image 0's tokens 0 (w 1) and 2 (w 1/3): O_ab = (0 + 2 ln 2) / 3, O_aa = ln 3 / 2; sqd the same for both tokens
    sqd = (2 * math.log(2.0) / 3 - math.log(3.0) / 2) ** 2
    assert torch.allclose(local[0], torch.tensor([sqd, 0.0, sqd, 0.0], dtype=torch.float64), atol=1e-7)
    wsum = (255 + 85) / 255.0
    assert torch.allclose(contrib[0], torch.tensor([sqd / wsum, 0.0, sqd / 3 / wsum, 0.0], dtype=torch.float64), atol=1e-7)
    assert abs(score - 0.5 * float(contrib.sum())) < 1e-12


def test_workspace_query_and_refusals_come_before_any_launch():
    """Every refusal of dsim_score_matrix_weights is decided on the host before anything is enqueued, so it is checked without a GPU
    (the pointers are never read)."""
    from diffsim_amd import _lib
    L = _lib.lib()
    B, H, N, D = 2, 4, 64, 32
    bf16 = _lib.DSIM_BF16
    wsb = L.dsim_score_matrix_weights_workspace_bytes
    need = int(wsb(3, 4, B, H, N, D, bf16))
    assert need > 0
    # the region matrix's workspace, then the biases [n_a + n_b][N up to whole 64-key tiles] and the byte sums
    assert need == int(L.dsim_score_matrix_regions_workspace_bytes(3, 4, B, H, N, D, bf16)) + 7 * 64 * 4 + 256
    assert int(wsb(3, 4, B, H, 65, D, bf16)) == int(L.dsim_score_matrix_regions_workspace_bytes(3, 4, B, H, 65, D, bf16)) + 7 * 128 * 4 + 256
    assert int(wsb(3, 4, B, H, N, D, _lib.DSIM_F32)) > need and int(wsb(3, 4, B, H, N, D, _lib.DSIM_F16)) == need
    big = 32767
    for args in ((3, 4, B, H, N, 24, bf16), (3, 4, B, H, N, D, 9), (3, 4, B, H, N, D, -1), (0, 4, B, H, N, D, bf16), (3, 0, B, H, N, D, bf16),
                 (3, 4, B, H, 0, D, bf16), (3, 4, 0, H, N, D, bf16), (65535, 1, 1, 1, 1, 16, bf16), (3, 2, 2, 32768, N, 16, bf16),
                 (big, big, 1, 1, 256, 16, bf16),
                 (1, 1, 1, 1, 8421505, 16, bf16)):                          # N 255 >= 2^31 (the features themselves still fit)
        assert wsb(*args) == 0, args
    # ((n_a + n_b) stride >= 2^31 cannot be reached alone: a set's features pass 2^31 elements first)
    assert L.dsim_score_matrix_regions_workspace_bytes(1, 1, 1, 1, 8421505, 16, bf16) > 0      # (the soft form's own refusal)
    fake = ctypes.c_void_p(0x10000)

    def go(n_a=3, n_b=4, H=H, N=N, D=D, dtype=bf16, sim=0, ws=need, weights_b=fake, out=fake):
        rc = L.dsim_score_matrix_weights(fake, fake, fake, fake, n_a, fake, fake, fake, weights_b, n_b, B, H, N, D, dtype, sim, out, None,
                                         None, fake, ws, None)
        return L.dsim_strerror(rc).lower()

    assert b"workspace" in go(ws=need // 2) and b"workspace" in go(ws=need - 257)
    for kw in (dict(dtype=9), dict(dtype=-1), dict(sim=2), dict(sim=-1), dict(D=24), dict(D=0), dict(n_a=0), dict(n_b=0), dict(n_a=-3),
               dict(n_a=65535, ws=1 << 44), dict(H=32768, ws=1 << 44), dict(n_a=1, n_b=1, H=1, N=8421505, D=16, ws=1 << 50),
               dict(weights_b=None), dict(out=None)):
        for dtype in ((bf16, _lib.DSIM_F16, _lib.DSIM_F32) if "dtype" not in kw else (kw["dtype"],)):
            assert b"invalid" in go(**{**kw, "dtype": dtype}), (kw, dtype)


# ---- engine.score_matrix_weights' own checks ------------------------------------------------------------------------------------------
def test_engine_checks_come_before_the_library(monkeypatch):
    from diffsim_amd import _lib, engine
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    N, H, D = 16, 2, 8
    fa = tuple(torch.zeros(2, 2, N, H * D) for _ in range(3))
    fb = tuple(torch.zeros(3, 2, N, H * D) for _ in range(3))
    wa, wb = torch.full((2, N), 255, dtype=torch.uint8), torch.full((3, N), 7, dtype=torch.uint8)
    with pytest.raises(_lib.DsimError, match="not on the GPU"):
        engine.score_matrix_weights(fa, fb, wa, wb, H)
    with pytest.raises(_lib.DsimError, match="weights_a must be uint8"):                       # (uint8 only, as pair_score_weights)
        engine.score_matrix_weights(fa, fb, wa.bool(), wb, H)
    with pytest.raises(_lib.DsimError, match="weights_b must be uint8"):
        engine.score_matrix_weights(fa, fb, wa, wb.float(), H)
    with pytest.raises(_lib.DsimError, match=r"weights_b must be \(n, N\) = \(3, 16\)"):
        engine.score_matrix_weights(fa, fb, wa, wb[:2], H)
    with pytest.raises(_lib.DsimError, match=r"weights_a must be \(n, N\)"):
        engine.score_matrix_weights(fa, fb, wa.view(2, 4, 4), wb, H)
    with pytest.raises(_lib.DsimError, match="weights_b must be contiguous"):
        engine.score_matrix_weights(fa, fb, wa, torch.zeros(N, 3, dtype=torch.uint8).T, H)
    with pytest.raises(_lib.DsimError, match="one geometry"):
        engine.score_matrix_weights(fa, tuple(t[:, :, :8] for t in fb), wa, wb, H)
    with pytest.raises(ValueError):
        engine.score_matrix_weights(fa, fb, wa, wb, H, "l1")


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_soft_masks_with_retrieval(capsys):
    from diffsim_amd.cli import FEATURE_METRICS, VIT_METRICS, arg_parse
    base = ["--dataset", "retrieval", "--image_path", "g", "--query_path", "q", "--out_path", "o", "--soft_masks"]
    for extra in (["--query_mask_path", "qm"], ["--gallery_mask_path", "gm"], ["--query_mask_path", "qm", "--gallery_mask_path", "gm"]):
        a = arg_parse(base + extra)
        assert a.soft_masks is True and a.text_soft is False and a.mask_path is None
        hard = vars(arg_parse([x for x in base if x != "--soft_masks"] + extra))
        assert {**hard, "soft_masks": True} == vars(a)                       # the flag changes nothing else of the namespace

    def refused(argv, named):
        with pytest.raises(SystemExit) as e:
            arg_parse(argv)
        assert e.value.code == 2, argv
        msg = capsys.readouterr().err.split("error:")[-1]                    # (the message, not the usage text above it)
        assert all(n in msg for n in named), (argv, msg)

    refused(base, ["--soft_masks", "--query_mask_path", "--gallery_mask_path"])                # no masks at all
    refused(base + ["--mask_path", "m"], ["--soft_masks", "--query_mask_path"])                # retrieval's partner is not --mask_path
    for m in sorted(VIT_METRICS) + sorted(FEATURE_METRICS):
        refused(base + ["--query_mask_path", "qm", "--metric", m], ["--soft_masks"])
    refused(base + ["--query_mask_path", "qm", "--taps", "up_blocks:0"], ["--taps"])
    # text-guided retrieval stays refused; the per-token outputs are accepted: they hold the soft forms
    refused(["--dataset", "retrieval", "--text_attn", "--text_soft"], ["--text_soft"])
    a = arg_parse(base + ["--query_mask_path", "qm", "--save_region_maps", "--save_region_matches"])
    assert a.soft_masks and a.save_region_maps and a.save_region_matches
    refused(base + ["--save_region_maps"], ["--soft_masks"])                                    # (still no masks at all)
    refused(base + ["--query_mask_path", "qm", "--save_maps"], ["--query_mask_path"])


# ---- retrieval's soft=True on a CPU stand-in ------------------------------------------------------------------------------------------
def _soft_cells(fa, fb, wa, wb, heads, sim):
    s = Soft64(*(torch.cat([a, b]) for a, b in zip(fa, fb)), torch.cat([wa, wb]), heads, torch.float32)
    n_a, n_b = wa.shape[0], wb.shape[0]
    return torch.tensor([[s.pair(i, n_a + j, sim) for j in range(n_b)] for i in range(n_a)], dtype=torch.float32)


def test_latent_matrix_soft_masks_reach_the_soft_matrix(monkeypatch):
    from diffsim_amd import retrieval as R
    from diffsim_amd._lib import DsimError
    calls = []

    def weights(fa, fb, wa, wb, heads, sim, return_status=False):
        assert wa.dtype == wb.dtype == torch.uint8 and wa.is_contiguous() and wb.is_contiguous()
        calls.append(("weights", wa.clone(), wb.clone()))
        return _soft_cells(fa, fb, wa, wb, heads, sim), torch.zeros(wa.shape[0], wb.shape[0], dtype=torch.int32)

    def regions(fa, fb, ma, mb, heads, sim, return_status=False):
        calls.append(("regions", ma.clone(), mb.clone()))
        r = Region64(*(torch.cat([a, b]) for a, b in zip(fa, fb)), torch.cat([ma, mb]), heads, torch.float32)
        n_a, n_b = ma.shape[0], mb.shape[0]
        s = torch.tensor([[r.pair(i, n_a + j, sim) for j in range(n_b)] for i in range(n_a)], dtype=torch.float32)
        return s, torch.zeros(n_a, n_b, dtype=torch.int32)

    asked = []
    monkeypatch.setattr(R, "score_matrix_weights", weights)
    monkeypatch.setattr(R, "score_matrix_regions", regions)
    monkeypatch.setattr(R, "score_matrix", lambda *a, **k: pytest.fail("the unmasked matrix"))
    monkeypatch.setattr(R, "score_matrix_weights_workspace_bytes", lambda *a: asked.append("weights") or 0)
    monkeypatch.setattr(R, "score_matrix_regions_workspace_bytes", lambda *a: asked.append("regions") or 0)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev=None: (1 << 40, 1 << 40))
    sc = _Scorer()
    g = torch.Generator().manual_seed(3)
    la, lb, nz = torch.randn(2, 4, 4, 4, generator=g), torch.randn(3, 4, 4, 4, generator=g), torch.randn(1, 4, 4, 4, generator=g)
    wA = torch.randint(0, 256, (2, 4, 4), generator=g).to(torch.uint8)
    wA[0] = 0                                                                # no weight at all: the whole image
    wB = [None, torch.rand(16, generator=g).numpy(), torch.rand(4, 4, generator=g) < 0.5]    # whole | floats in [0, 1] | bool
    both = R.score_latent_matrix(sc, la, lb, nz, nz, "p", batch=2, masks_a=wA, masks_b=wB, soft=True)
    assert [c[0] for c in calls] == ["weights", "weights"] and set(asked) == {"weights"}     # two gallery chunks, the soft query
    assert (calls[0][1][0] == 255).all() and torch.equal(calls[0][1][1], wA[1].flatten())
    assert calls[0][2].shape == (2, 16) and calls[1][2].shape == (1, 16)     # the gallery's weights sliced as its latents are
    assert (calls[0][2][0] == 255).all()
    assert torch.equal(calls[0][2][1], torch.floor(255.0 * torch.as_tensor(wB[1]).double() + 0.5).to(torch.uint8))
    assert torch.equal(calls[1][2][0], wB[2].flatten().to(torch.uint8) * 255)
    assert torch.isfinite(both).all()
    one = R.score_latent_matrix(sc, la, lb, nz, nz, "p", batch=3, masks_a=wA, masks_b=wB, soft=True)
    assert torch.equal(one, both)                                            # a chunked gallery equals the unchunked one
    calls.clear()
    only_b = R.score_latent_matrix(sc, la, lb, nz, nz, "p", masks_b=wB, soft=True)
    assert calls[0][0] == "weights" and (calls[0][1] == 255).all() and not torch.equal(only_b, both)
    # bool masks: soft and hard are the same cells (Soft64 on 0 / 255 is Region64)
    calls.clear()
    mA, mB = torch.rand(2, 4, 4, generator=g) < 0.5, torch.rand(3, 16, generator=g) < 0.5
    mA[:, 0, 0] = True
    mB[:, 0] = True
    soft = R.score_latent_matrix(sc, la, lb, nz, nz, "p", masks_a=mA, masks_b=mB, soft=True)
    hard = R.score_latent_matrix(sc, la, lb, nz, nz, "p", masks_a=mA, masks_b=mB)
    assert [c[0] for c in calls] == ["weights", "regions"] and torch.equal(soft, hard)
    with pytest.raises(ValueError, match="masks_a"):
        R.score_latent_matrix(sc, la, lb, nz, nz, "p", masks_a=wA[:1], soft=True)
    with pytest.raises(ValueError, match="token grid"):
        R.score_latent_matrix(sc, la, lb, nz, nz, "p", masks_b=[None, torch.ones(3, 3), None], soft=True)
    with pytest.raises(DsimError, match="masks_a"):
        R.score_latent_matrix(sc, la, lb, nz, nz, "p", soft=True)           # nothing to weigh
    with pytest.raises(TypeError):
        R.score_latent_matrix(sc, la, lb, nz, nz, "p", "up_blocks", 0, 600, "cosine", None, False, wA, None, True)      # keyword-only
