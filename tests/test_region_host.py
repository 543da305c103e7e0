"""Region scores, host side (no GPU): the C ABI's two entry points and their refusals, tests/_region64.py itself (full regions are
Tail64's pair; a hand-written masked softmax), token masks from mask images, the --mask_path lookup and command line, and the
triplet harness with and without masks on CPU stand-ins."""
import glob
import os
import re

import numpy as np
import pytest
import torch

from tests._region64 import Region64, regions64
from tests._tail64 import Tail64, heads64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMGS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "g1_img_*.png")))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_region_entry_points():
    hdr = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    assert re.search(r"size_t\s+dsim_pair_score_regions_workspace_bytes\s*\(\s*int n_feat,\s*int n_pairs,\s*int B,\s*int H,\s*int N,"
                     r"\s*int D\)", hdr)
    assert re.search(r"#define\s+DSIM_ABI_VERSION\s+7\b", hdr)             # additive: the version stays
    from diffsim_amd import _lib
    assert _lib.ABI_VERSION == 7
    assert len(_lib.SYMBOLS["dsim_pair_score_regions_workspace_bytes"][1]) == 6
    assert len(_lib.SYMBOLS["dsim_pair_score_regions"][1]) == 20
    decl = re.search(r"int\s+dsim_pair_score_regions\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 20


def test_refusals_come_before_any_launch():
    """Every refusal of dsim_pair_score_regions is decided on the host before anything is enqueued, so it is checked without a GPU
    (the pointers are never read): the workspace query's zeros, a short workspace, a bad dtype, similarity or head dim, no pairs, no
    feature images, and grids past 65535."""
    import ctypes
    from diffsim_amd import _lib
    L = _lib.lib()
    B, H, N, D = 2, 4, 64, 32
    wsb = L.dsim_pair_score_regions_workspace_bytes
    need = int(wsb(3, 2, B, H, N, D))
    assert need >= 3 * N * 4 + 3 * 4 + 2 * 2 * B * H * 4 * 4
    for args in ((0, 2, B, H, N, D), (3, 0, B, H, N, D), (3, 2, B, H, N, 24), (3, 2, B, H, N, 0), (3, 2, B, H, 0, D),
                 (3, 32768, B, H, N, D), (3, 2, 2, 32768, N, D), (3, 2, 0, H, N, D)):
        assert wsb(*args) == 0, args
    assert wsb(3, 32767, B, H, N, D) > 0 and wsb(3, 2, 1, 65535, N, D) > 0
    fake = ctypes.c_void_p(0x10000)

    def go(n_feat=3, n=2, H=H, N=N, D=D, dtype=_lib.DSIM_BF16, sim=0, ws=need):
        rc = L.dsim_pair_score_regions(fake, fake, fake, fake, n_feat, fake, fake, n, B, H, N, D, dtype, sim, fake, None, None, fake,
                                       ws, None)
        return L.dsim_strerror(rc).lower()

    assert b"workspace" in go(ws=need // 2)
    assert b"workspace" in go(ws=need - 257)          # (the query adds 256 bytes of alignment slack; the pointer here is aligned)
    for kw in (dict(dtype=9), dict(dtype=-1), dict(sim=2), dict(sim=-1), dict(D=24), dict(D=0), dict(n=0), dict(n=-3), dict(n_feat=0),
               dict(n=32768, ws=1 << 40), dict(H=32768, ws=1 << 40)):
        for dtype in ((_lib.DSIM_BF16, _lib.DSIM_F16, _lib.DSIM_F32) if "dtype" not in kw else (kw["dtype"],)):
            assert b"invalid" in go(**{**kw, "dtype": dtype}), (kw, dtype)
    rc = L.dsim_pair_score_regions(fake, fake, fake, None, 3, fake, fake, 2, B, H, N, D, _lib.DSIM_BF16, 0, fake, None, None, fake, need,
                                   None)
    assert b"invalid" in L.dsim_strerror(rc).lower()                        # no mask


# ---- tests/_region64.py ---------------------------------------------------------------------------------------------------------------
def _feats(n, seed, dtype, N, H, D, B=2):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(n, B, N, H * D, generator=g).to(dtype) for _ in range(3))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("sim", ["cosine", "mse"])
def test_region64_with_full_regions_is_tail64(dtype, sim):
    N, H, D = 49, 2, 16
    q, k, v = _feats(3, 5, dtype, N, H, D)
    full = torch.ones(3, N, dtype=torch.bool)
    t, r = Tail64(q, k, v, H, dtype), Region64(q, k, v, full, H, dtype)
    for a, b in ((0, 1), (1, 2), (2, 2)):
        assert r.pair(a, b, sim) == t.pair(a, b, sim)[0]
    assert regions64(q, k, v, full.to(torch.uint8) * 255, [0, 1], [1, 2], H, sim, dtype) == [t.pair(0, 1, sim)[0], t.pair(1, 2, sim)[0]]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("sim", ["cosine", "mse"])
def test_region64_is_a_masked_softmax(dtype, sim):
    """Written out by hand in float64: -inf on the off keys, the off queries dropped, the outputs rounded to the pipeline dtype."""
    N, H, D, B = 36, 2, 8, 2
    q, k, v = _feats(2, 9, dtype, N, H, D)
    g = torch.Generator().manual_seed(1)
    mask = torch.rand(2, N, generator=g) < 0.4
    mask[0, 3] = mask[1, 30] = True

    def attn(i, j):
        qq, kk, vv = heads64(q[i], H), heads64(k[j], H), heads64(v[j], H)
        s = qq @ kk.transpose(-1, -2) / D ** 0.5
        s = s.masked_fill(~mask[j].view(1, 1, 1, N), float("-inf"))
        o = (torch.softmax(s, -1) @ vv).to(dtype).double()
        return o[:, :, mask[i]]                     # (B, H, |R_i|, D)

    want = 0.0
    for a, b in ((0, 1), (1, 0)):
        x, y = attn(a, b), attn(a, a)
        if sim == "cosine":
            want += float((x * y).sum() / (x.pow(2).sum().sqrt().clamp_min(1e-8) * y.pow(2).sum().sqrt().clamp_min(1e-8)))
        else:
            want += float(((x - y) ** 2).sum() / (B * H * int(mask[a].sum()) * D))
    got = regions64(q, k, v, mask, [0], [1], H, sim, dtype)[0]
    assert abs(got - 0.5 * want) <= 1e-12 * max(1.0, abs(want)), (got, 0.5 * want)


# ---- token masks ----------------------------------------------------------------------------------------------------------------------
def _img(a, mode="L"):
    from PIL import Image
    return Image.fromarray(np.asarray(a, dtype=np.uint8), "L").convert(mode)


def test_token_mask_thresholds_the_area_average_at_128():
    from diffsim_amd.regions import token_mask
    a = np.zeros((8, 8), np.uint8)
    a[0:4, 0:2] = 254           # cell (0, 0) of a 2 x 2 grid, half covered at 254: average 127 -> off
    a[0:4, 4:6] = 255           # cell (0, 1), half covered at 255: average 127.5, stored as 128 -> on
    a[4:8, 0:4] = 128           # cell (1, 0), wholly 128 -> on
    a[4:8, 4:8] = 127           # cell (1, 1), wholly 127 -> off
    m = token_mask(_img(a), (2, 2))
    assert m.dtype == torch.bool and m.tolist() == [[False, True], [True, False]]


def test_token_mask_of_an_all_black_mask_is_the_whole_image():
    from diffsim_amd.regions import load_token_masks, token_mask
    assert token_mask(_img(np.zeros((16, 16))), (4, 4)).all()
    assert token_mask(_img(np.full((16, 16), 100)), (4, 4)).all()             # (nothing reaches 128)
    assert load_token_masks([None, None], (3, 3)).shape == (2, 3, 3) and load_token_masks([None], (3, 3)).all()


@pytest.mark.parametrize("mode", ["1", "L", "RGBA", "RGB", "P"])
def test_token_mask_takes_any_mode(mode):
    from diffsim_amd.regions import token_mask
    a = np.zeros((12, 12), np.uint8)
    a[:6, 6:] = 255
    assert token_mask(_img(a, mode), (2, 2)).tolist() == [[False, True], [False, False]]


def test_token_mask_of_a_non_square_source_and_from_files(tmp_path):
    from diffsim_amd.regions import as_token_mask, load_token_masks, token_mask
    a = np.zeros((30, 80), np.uint8)            # 30 rows, 80 columns
    a[:, 40:] = 255
    a[:15, :20] = 255
    want = [[True, False, True, True], [False, False, True, True]]
    assert token_mask(_img(a), (2, 4)).tolist() == want
    p = tmp_path / "m.png"
    _img(a).save(p)
    assert as_token_mask(str(p), (2, 4)).tolist() == want
    assert load_token_masks([str(p), None], (2, 4)).tolist() == [want, [[True] * 4] * 2]
    assert as_token_mask(np.array(want), (2, 4)).tolist() == want and as_token_mask(torch.tensor(want).flatten(), (2, 4)).tolist() == want
    with pytest.raises(ValueError, match="token grid"):
        as_token_mask(np.ones((3, 3), bool), (2, 4))


# ---- the mask lookup and the command line ---------------------------------------------------------------------------------------------
def test_mask_lookup_prefers_png_then_the_image_name_and_counts_the_missing(tmp_path):
    from diffsim_amd.regions import mask_path_for, triplet_mask_paths
    img, msk = tmp_path / "img", tmp_path / "msk"
    for rel in ("a/x.jpg", "a/y.jpg", "b/z.png", "b/w.jpeg"):
        (img / rel).parent.mkdir(parents=True, exist_ok=True)
        (img / rel).write_bytes(b"")
    for rel in ("a/x.png", "a/x.jpg", "a/y.jpg", "b/z.png"):
        (msk / rel).parent.mkdir(parents=True, exist_ok=True)
        (msk / rel).write_bytes(b"")
    at = lambda rel: str(img / rel)                                         # noqa: E731
    assert mask_path_for(at("a/x.jpg"), str(img), str(msk)) == str(msk / "a/x.png")         # name.png first
    assert mask_path_for(at("a/y.jpg"), str(img), str(msk)) == str(msk / "a/y.jpg")         # else name.ext
    assert mask_path_for(at("b/z.png"), str(img), str(msk)) == str(msk / "b/z.png")
    assert mask_path_for(at("b/w.jpeg"), str(img), str(msk)) is None
    trip = [(at("a/x.jpg"), at("a/y.jpg"), at("b/w.jpeg"), "p"), (at("b/w.jpeg"), at("b/z.png"), at("a/x.jpg"), "p")]
    masks, missing = triplet_mask_paths(trip, str(img), str(msk))
    assert masks == [(str(msk / "a/x.png"), str(msk / "a/y.jpg"), None), (None, str(msk / "b/z.png"), str(msk / "a/x.png"))]
    assert missing == 1                                                      # distinct images, not occurrences


def test_mask_path_is_for_the_one_tap_cute_and_nights_runs(capsys):
    from diffsim_amd.cli import arg_parse
    a = arg_parse(["--dataset", "cute", "--mask_path", "m"])
    assert a.mask_path == "m" and a.use_mask is True                        # implied
    assert arg_parse(["--dataset", "nights", "--mask_path", "m", "--use_mask"]).use_mask is True
    b = arg_parse(["--use_mask"])                                           # accepted and without effect, as before
    assert b.use_mask is True and b.mask_path is None
    assert arg_parse([]).use_mask is False
    for extra in (["--dataset", "sref"], ["--dataset", "retrieval"], ["--dataset", "cute", "--taps", "up_blocks:0"]):
        with pytest.raises(SystemExit) as e:
            arg_parse(extra + ["--mask_path", "m"])
        assert e.value.code == 2
        assert "--mask_path" in capsys.readouterr().err


# ---- the harness on CPU stand-ins -------------------------------------------------------------------------------------------------------
def _stub_pair_score(q, k, v, ia, ib, heads, similarity="cosine", return_status=False):
    t = Tail64(q, k, v, heads, q.dtype)
    s = torch.tensor([t.pair(a, b, similarity)[0] for a, b in zip(ia.tolist(), ib.tolist())], dtype=torch.float32)
    return (s, torch.zeros(len(s), dtype=torch.int32)) if return_status else s


def _stub_pair_score_regions(q, k, v, mask, ia, ib, heads, similarity="cosine", return_status=False, return_counts=False):
    s = torch.tensor(regions64(q, k, v, mask, ia, ib, heads, similarity, q.dtype), dtype=torch.float32)
    return (s, torch.zeros(len(s), dtype=torch.int32)) if return_status else s


def _stub_scorer(monkeypatch):
    from tests._fakes import FakeVAE
    from tests.test_chunk_sizes_host import make
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev=None: (10000 << 30, 20000 << 30))
    s, eng, _, _, _ = make("sd15")
    s.vae = FakeVAE()
    eng.heads, eng.tokens = 4, 64

    def feats(lat, nz, *a, **k):                    # (n, 4, 16, 16) -> q, k, v [n][2][64][16]: an 8 x 8 grid, 4 heads x 4
        x = (lat + 0.1 * nz).reshape(lat.shape[0], 64, 16)
        q = torch.stack([x, x.flip(1)], 1).contiguous()
        return q, (q * 0.5 + 0.1).contiguous(), (q - 0.2).contiguous()
    s.features = feats
    return s


def test_triplets_without_masks_take_the_unmasked_path(monkeypatch):
    """masks=None: the pair tail with today's arguments, the region tail never; a mask triple of Nones: the region tail over
    full masks, the same scores."""
    from diffsim_amd import harness as H
    calls = []

    def pair(*a, **k):
        calls.append(("pair", len(a), sorted(k)))
        return _stub_pair_score(*a, **k)

    def region(*a, **k):
        calls.append(("region", a[3].clone()))
        return _stub_pair_score_regions(*a, **k)
    monkeypatch.setattr(H, "pair_score", pair)
    monkeypatch.setattr(H, "pair_score_regions", region)
    s = _stub_scorer(monkeypatch)
    a, b, c, d = IMGS
    trip = [(a, b, c, "p"), (d, c, a, "p"), (b, a, d, "p")]
    l0, r0, bad0 = H.score_path_triplets(s, trip, 128, "up_blocks", [0], 600, 2334, "cosine", batch_triplets=2, unet_triplets=2)
    assert [c[0] for c in calls] == ["pair", "pair"] and all(c[1:] == (7, ["return_status"]) for c in calls)
    del calls[:]
    l1, r1, bad1 = H.score_path_triplets(s, trip, 128, "up_blocks", [0], 600, 2334, "cosine", batch_triplets=2, unet_triplets=2,
                                         masks=[(None, None, None)] * 3)
    assert [c[0] for c in calls] == ["region", "region"] and calls[0][1].shape == (6, 64) and calls[1][1].shape == (3, 64)
    assert all(bool(c[1].all()) for c in calls)
    assert torch.equal(l0, l1) and torch.equal(r0, r1) and bad0 == bad1 == 0
    with pytest.raises(ValueError, match="mask triples"):
        H.score_path_triplets(s, trip, 128, "up_blocks", [0], 600, 2334, "cosine", masks=[(None, None, None)])


def test_triplet_masks_lie_as_the_chunk_images_do(monkeypatch, tmp_path):
    """(ref, left, right) masks reach the tail interleaved like stack_rows' images; each side's score is the region score of its
    two images and masks (what region_score computes through score_path_pair_regions)."""
    from diffsim_amd import harness as H, regions as R
    monkeypatch.setattr(H, "pair_score_regions", _stub_pair_score_regions)
    monkeypatch.setattr(R, "pair_score_regions", _stub_pair_score_regions)
    s = _stub_scorer(monkeypatch)
    a, b, c, d = IMGS
    g = torch.Generator().manual_seed(2)
    arrays = [torch.rand(8, 8, generator=g) < 0.5 for _ in range(5)]
    png = tmp_path / "left.png"
    big = np.zeros((64, 64), np.uint8)
    big[:32] = 255
    _img(big).save(png)
    masks = [(arrays[0], str(png), arrays[1]), (None, arrays[2], None), (arrays[3], arrays[4], str(png))]
    trip = [(a, b, c, "p"), (d, c, a, "p"), (b, a, d, "p")]
    sl, sr, bad = H.score_path_triplets(s, trip, 128, "up_blocks", [0], 600, 2334, "mse", batch_triplets=3, unet_triplets=2, masks=masks)
    assert bad == 0
    for i, (t, m) in enumerate(zip(trip, masks)):
        wl = s.region_score(t[0], t[1], m[0], m[1], 128, "p", "up_blocks", [0], 600, seed=2334, similarity="mse")
        wr = s.region_score(t[0], t[2], m[0], m[2], 128, "p", "up_blocks", [0], 600, seed=2334, similarity="mse")
        assert wl.shape == (1,) and torch.equal(wl[0], sl[i]) and torch.equal(wr[0], sr[i]), i
    with pytest.raises(ValueError, match="no token on"):
        R.score_latent_pair_regions(s, torch.zeros(2, 4, 16, 16), torch.zeros(2, 4, 16, 16), torch.zeros(1, 4, 16, 16),
                                    torch.zeros(1, 4, 16, 16), torch.ones(2, 8, 8, dtype=torch.bool), torch.zeros(2, 64, dtype=torch.bool),
                                    "p", "up_blocks", 0, 600)
    with pytest.raises(ValueError, match="token grid"):
        R.score_latent_pair_regions(s, torch.zeros(2, 4, 16, 16), torch.zeros(2, 4, 16, 16), torch.zeros(1, 4, 16, 16),
                                    torch.zeros(1, 4, 16, 16), torch.ones(2, 4, 4, dtype=torch.bool), torch.ones(2, 4, 4, dtype=torch.bool),
                                    "p", "up_blocks", 0, 600)


# ---- the one-pair path methods: one body on Scorer, the kinds' facts reach the module functions -----------------------------------------
def _kinds():
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.diffsim_dit import diffsim_DiT
    from diffsim_amd.diffsim_xl import diffsim_xl
    # (kind, the --target_layer given, (prompt, block, layer) the module functions get, hip_vae, batch_pairs)
    return [(DiffSim, [0], ("p", "up_blocks", 0), True, None), (diffsim_xl, [0, 1, 2], ("p", "up_blocks", [0, 1, 2]), False, None),
            (diffsim_DiT, [3], (None, "none", [3]), False, 32)]


@pytest.mark.parametrize("which", [0, 1, 2], ids=["DiffSim", "diffsim_xl", "diffsim_DiT"])
def test_path_methods_hand_the_kinds_facts_to_the_module_functions(monkeypatch, which):
    """Every one-pair path method, once per kind: the prompt / block / layer, hip_vae and batch_pairs that arrive at the module
    function are the kind's -- DiffSim: the layer through _norm_layer, the HIP VAE, no batch; diffsim_xl: the flag pair untouched,
    no HIP VAE, no batch; diffsim_DiT: (None, "none", [layer]), no HIP VAE, 32 pairs."""
    import inspect
    from diffsim_amd import align, inputs, maps, regions, textattn, transfer
    cls, layer, (prompt, block, tap_layer), hip_vae, batch = _kinds()[which]
    log = []

    def record(mod, name, result=None):
        sig = inspect.signature(getattr(mod, name))

        def fake(*a, **k):
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            log.append((name, dict(bound.arguments)))
            return result
        monkeypatch.setattr(mod, name, fake)
    z = torch.zeros(1, 4, 2, 2)
    for mod, name in ((regions, "score_path_pair_regions"), (regions, "score_path_pair_weights"), (maps, "score_path_pair_maps"),
                      (align, "score_path_pair_alignment"), (textattn, "score_path_pairs_text"), (textattn, "text_attention_maps"),
                      (transfer, "score_path_pairs_exemplar"), (transfer, "path_transferred_region")):
        record(mod, name)
    record(inputs, "path_latents", ((z, z), z, z))
    s = object.__new__(cls)
    if hip_vae:                                                             # DiffSim draws one call's latents its own way
        s._path_pair_latents = lambda *a: (z, z, z, z)
    head = ("a.png", "b.png")
    tail = (128, "p", "up_blocks", layer, 600)
    masked = ("region_score", "soft_region_score", "region_similarity_maps", "soft_region_similarity_maps", "region_alignment",
              "soft_region_alignment")
    for name in masked:
        getattr(s, name)(*head, "ma", "mb", *tail, 7, *(() if "alignment" in name else ("mse",)))
    s.alignment(*head, *tail, 7)
    s.exemplar_region_score(*head, "ma", *tail, 7, "mse", 1.5, True)
    s.transferred_region(*head, "ma", *tail, 7, 1.5, True)
    if which == 2:
        for name in ("text_region_score", "text_attention_map"):
            with pytest.raises(NotImplementedError, match="diffsim_DiT has no text conditioning"):
                getattr(s, name)(*head, *tail, 7)
    else:
        s.text_region_score(*head, *tail, 7, "mse", ["cat"], 1.25)
        s.text_attention_map(*head, *tail, 7)
    want = ["score_path_pair_regions", "score_path_pair_weights", "score_path_pair_maps", "score_path_pair_maps",
            "score_path_pair_alignment", "score_path_pair_alignment", "score_path_pair_alignment", "score_path_pairs_exemplar",
            "path_transferred_region"] + ([] if which == 2 else ["score_path_pairs_text"] + ["path_latents"] * (not hip_vae) +
                                          ["text_attention_maps"])
    assert [n for n, _ in log] == want
    for name, got in log:
        if name == "path_latents":
            assert got["hip_vae"] is False and got["rows"] == [head] and got["seed"] == 7 and got["img_size"] == 128
            continue
        assert (got["prompt"], got["target_block"], got["target_layer"]) == (prompt, block, tap_layer), name
        assert got["target_step"] == 600 and got["scorer"] is s, name
        if name == "text_attention_maps":
            assert got["lat"].shape[0] == 2 and got["batch"] is None
            continue
        assert got["hip_vae"] is hip_vae and got["seed"] == 7 and got["img_size"] == 128, name
        if name != "score_path_pairs_text":
            assert got["batch_pairs"] == batch, name
    by = lambda name: [g for n, g in log if n == name]                       # noqa: E731
    assert all(g["pairs"] == [head] and g["masks"] == [("ma", "mb")] and g["similarity"] == "mse"
               for n, g in log if n in ("score_path_pair_regions", "score_path_pair_weights", "score_path_pair_maps"))
    assert [g["soft"] for g in by("score_path_pair_maps")] == [False, True]
    assert [(g["masks"], g["soft"]) for g in by("score_path_pair_alignment")] == [([("ma", "mb")], False), ([("ma", "mb")], True), (None, False)]
    ex, tr = by("score_path_pairs_exemplar")[0], by("path_transferred_region")[0]
    assert ex["masks_a"] == ["ma"] and (ex["similarity"], ex["rel_threshold"], ex["soft"], ex["return_regions"]) == ("mse", 1.5, True, False)
    assert (tr["image_A"], tr["image_B"], tr["mask_A"], tr["rel_threshold"], tr["soft"]) == (*head, "ma", 1.5, True)
    if which != 2:
        tx = by("score_path_pairs_text")[0]
        assert (tx["similarity"], tx["words"], tx["rel_threshold"], tx["weights"], tx["batch_pairs"], tx["soft"]) == \
            ("mse", ["cat"], 1.25, None, None, False)


def test_hard_region_tails_refuse_a_strided_mask(monkeypatch):
    """A mask that is not contiguous would be read as if dense: the four hard forms refuse it as the soft forms do, before anything
    needs a device."""
    from diffsim_amd import _lib, engine
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    N, H, D = 16, 2, 8
    q, k, v = (torch.zeros(3, 2, N, H * D) for _ in range(3))
    ia = torch.zeros(1, dtype=torch.int32)
    m = torch.ones(3, N, dtype=torch.bool)
    strided = m.t().contiguous().t()
    assert strided.shape == m.shape and not strided.is_contiguous()
    for call in (lambda mk: engine.pair_score_regions(q, k, v, mk, ia, ia, H), lambda mk: engine.pair_score_maps_regions(q, k, v, mk, ia, ia, H),
                 lambda mk: engine.pair_align_regions(q, k, mk, ia, ia, H),
                 lambda mk: engine.score_matrix_regions((q, k, v), (q, k, v), mk, m, H),
                 lambda mk: engine.score_matrix_regions((q, k, v), (q, k, v), m, mk, H)):
        with pytest.raises(_lib.DsimError, match="contiguous"):
            call(strided)
        with pytest.raises(_lib.DsimError, match="not on the GPU"):         # (a dense mask gets as far as the device requirement)
            call(m)
