"""Soft region scores, host side (no GPU): tests/_soft64.py itself (0/255 weights are tests/_region64.py exactly; a hand-written
weighted softmax), token weights from mask images, the C ABI's two entry points, the soft text weights' rule and the command line."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests._region64 import Region64
from tests._soft64 import Soft64, soft64
from tests._tail64 import heads64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _feats(n, seed, dtype, N, H, D, B=2):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(n, B, N, H * D, generator=g).to(dtype) for _ in range(3))


# ---- tests/_soft64.py -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("sim", ["cosine", "mse"])
def test_soft64_with_binary_weights_is_region64_exactly(dtype, sim):
    N, H, D = 49, 2, 16
    q, k, v = _feats(3, 5, dtype, N, H, D)
    g = torch.Generator().manual_seed(2)
    mask = torch.rand(3, N, generator=g) < 0.5
    mask[2] = True
    w = mask.to(torch.uint8) * 255
    nan = tuple(t.clone() for t in (q, k, v))
    for t in nan:
        t.transpose(1, 2)[~mask] = float("nan")                 # (a zero-weight row is index-selected away, never touched)
    s, r = Soft64(*nan, w, H, dtype), Region64(q, k, v, mask, H, dtype)
    for a, b in ((0, 1), (1, 2), (2, 2), (2, 0)):
        assert s.pair(a, b, sim) == r.pair(a, b, sim)
    w[1] = 0
    assert np.isnan(soft64(q, k, v, w, [0, 0], [1, 2], H, sim, dtype)[0]) and soft64(q, k, v, w, [0], [2], H, sim, dtype)[0] == r.pair(0, 2, sim)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("sim", ["cosine", "mse"])
def test_soft64_is_a_weighted_softmax(dtype, sim):
    """Written out by hand in float64 on the whole token grid: softmax(logits + log w) with log 0 = -inf, the outputs rounded to the
    pipeline dtype, the query weight on every sum, the mse count B H D sum(w)."""
    N, H, D, B = 36, 2, 8, 2
    q, k, v = _feats(2, 9, dtype, N, H, D)
    g = torch.Generator().manual_seed(1)
    m = torch.randint(0, 256, (2, N), generator=g).to(torch.uint8)
    m[:, ::3] = 0
    m[0, 3], m[1, 30] = 1, 255
    w = m.double() / 255.0

    def attn(i, j):
        qq, kk, vv = heads64(q[i], H), heads64(k[j], H), heads64(v[j], H)
        s = qq @ kk.transpose(-1, -2) / D ** 0.5 + torch.log(w[j]).view(1, 1, 1, N)
        return (torch.softmax(s, -1) @ vv).to(dtype).double()                   # (B, H, N, D), every query row

    want = 0.0
    for a, b in ((0, 1), (1, 0)):
        x, y, wa = attn(a, b), attn(a, a), w[a].view(1, 1, N, 1)
        if sim == "cosine":
            want += float((wa * x * y).sum() / ((wa * x * x).sum().sqrt().clamp_min(1e-8) * (wa * y * y).sum().sqrt().clamp_min(1e-8)))
        else:
            want += float((wa * (x - y) ** 2).sum() / (B * H * D * (float(m[a].long().sum()) / 255.0)))
    got = soft64(q, k, v, m, [0], [1], H, sim, dtype)[0]
    assert abs(got - 0.5 * want) <= 1e-12 * max(1.0, abs(want)), (got, 0.5 * want)


# ---- token weights --------------------------------------------------------------------------------------------------------------------
def _img(a, mode="L"):
    from PIL import Image
    return Image.fromarray(np.asarray(a, dtype=np.uint8), "L").convert(mode)


def test_token_weights_are_the_box_bytes():
    from PIL import Image
    from diffsim_amd.regions import token_weights
    a = np.zeros((8, 8), np.uint8)
    a[0:4, 0:2] = 254           # cell (0, 0) of a 2 x 2 grid, half covered at 254: 127
    a[0:4, 4:6] = 255           # cell (0, 1), half covered at 255: 127.5, stored as 128
    a[4:8, 0:4] = 128
    a[4:8, 4:6] = 255           # cell (1, 1), half covered too
    t = token_weights(_img(a), (2, 2))
    assert t.dtype == torch.uint8 and t.tolist() == [[127, 128], [128, 128]]
    g = np.random.default_rng(3)
    for size, grid in (((64, 48), (8, 6)), ((30, 80), (2, 4)), ((50, 50), (7, 7))):
        im = _img(g.integers(0, 256, size))
        want = np.asarray(im.resize((grid[1], grid[0]), Image.BOX))
        assert token_weights(im, grid).numpy().tolist() == want.tolist()
        assert token_weights(im.convert("RGB"), grid).numpy().tolist() == want.tolist()


def test_token_weights_at_128_are_the_token_mask():
    from diffsim_amd.regions import token_mask, token_weights
    g = np.random.default_rng(7)
    for i in range(12):
        blocks = (g.random((8, 6)) < 0.5) * 255
        a = np.kron(blocks, np.ones((8, 8))) if i % 2 else np.kron(blocks, np.ones((5, 7))) * (g.random((40, 42)) < 0.7)
        for grid in ((4, 3), (8, 6), (5, 5), (16, 16)):
            w, m = token_weights(_img(a), grid), token_mask(_img(a), grid)
            assert torch.equal(w >= 128, m) or not bool((w >= 128).any()), (i, grid)
            if not bool((w >= 128).any()):
                assert m.all()                                                   # (token_mask's fallback: nothing reaches 128)
    zero = token_weights(_img(np.zeros((16, 16))), (4, 4))                       # the all-zero fallback: the whole image
    assert zero.dtype == torch.uint8 and zero.tolist() == [[255] * 4] * 4
    assert torch.equal(zero >= 128, token_mask(_img(np.zeros((16, 16))), (4, 4)))
    assert token_weights(_img(np.full((16, 16), 100)), (4, 4)).tolist() == [[100] * 4] * 4      # (soft: 100 stays 100)


def test_as_token_weights_takes_every_form(tmp_path):
    from diffsim_amd.regions import as_token_weights, token_weights
    a = np.zeros((30, 80), np.uint8)
    a[:, 40:] = 255
    a[:15, :20] = 200
    want = token_weights(_img(a), (2, 4)).tolist()
    assert want == [[200, 0, 255, 255], [0, 0, 255, 255]]
    p = tmp_path / "m.png"
    _img(a).save(p)
    assert as_token_weights(str(p), (2, 4)).tolist() == want and as_token_weights(p, (2, 4)).tolist() == want          # a path
    assert as_token_weights(_img(a), (2, 4)).tolist() == want                                                           # a PIL image
    b = np.array(want, dtype=np.uint8)
    assert as_token_weights(b, (2, 4)).tolist() == want and as_token_weights(torch.tensor(b).flatten(), (2, 4)).tolist() == want
    f = np.array([[0.0, 1.0, 0.5, 0.25], [1 / 255, 0.999, 0.002, 0.1]])
    assert as_token_weights(f, (2, 4)).tolist() == [[0, 255, 128, 64], [1, 255, 1, 26]]                   # round(255 w)
    assert as_token_weights(torch.tensor(f, dtype=torch.float32), (2, 4)).dtype == torch.uint8
    assert as_token_weights(np.array(want) > 0, (2, 4)).tolist() == [[255, 0, 255, 255], [0, 0, 255, 255]]
    assert as_token_weights(None, (2, 4)).tolist() == [[255] * 4] * 2
    with pytest.raises(ValueError, match="token grid"):
        as_token_weights(np.ones((3, 3), np.uint8), (2, 4))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        as_token_weights(np.full((2, 4), 1.5), (2, 4))


# ---- the soft text weights ----------------------------------------------------------------------------------------------------------------
def test_soft_token_bytes_rule():
    from diffsim_amd.textattn import soft_token_bytes
    s = torch.tensor([[0.0, 1.0, 2.0, 5.0], [1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0], [1.0, float("nan"), 1.0, 1.0]])
    hard = lambda thr: (s >= thr * s.mean(1, keepdim=True)).to(torch.uint8)                     # noqa: E731
    b = soft_token_bytes(s, hard(1.0), 1.0)
    assert b.dtype == torch.uint8
    assert b[0].tolist() == [0, 128, 255, 255]                  # mean 2: 255 s / 2 rounded half up, clamped; the hard-on tokens 255
    assert b[1].tolist() == [255] * 4 and b[2].tolist() == [255] * 4 and b[3].tolist() == [255] * 4
    assert soft_token_bytes(s, hard(0.0), 0.0).tolist() == [[255] * 4] * 4                     # threshold 0: the whole image
    b2 = soft_token_bytes(s, hard(2.0), 2.0)
    assert b2[0].tolist() == [0, 64, 128, 255] and b2[1].tolist() == [128] * 4
    on = hard(1.0).bool() & torch.isfinite(s).all(1, keepdim=True)
    assert (b[on] == 255).all()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_weights_entry_points():
    hdr = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    assert re.search(r"size_t\s+dsim_pair_score_weights_workspace_bytes\s*\(\s*int n_feat,\s*int n_pairs,\s*int B,\s*int H,\s*int N,"
                     r"\s*int D\)", hdr)
    assert re.search(r"#define\s+DSIM_ABI_VERSION\s+7\b", hdr)             # additive: the version stays
    from diffsim_amd import _lib
    assert _lib.ABI_VERSION == 7
    assert len(_lib.SYMBOLS["dsim_pair_score_weights_workspace_bytes"][1]) == 6
    assert len(_lib.SYMBOLS["dsim_pair_score_weights"][1]) == 20
    decl = re.search(r"int\s+dsim_pair_score_weights\s*\(([^;]*)\)\s*;", hdr).group(1)
    args = re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")
    assert len(args) == 20 and "uint8_t* weights" in args[3] and "weight_sums" in args[16]
    L = _lib.lib()
    assert L.dsim_version() == 7
    assert L.dsim_pair_score_weights_workspace_bytes(3, 2, 2, 4, 64, 32) > 0
    assert L.dsim_pair_score_weights_workspace_bytes(3, 2, 2, 4, 64, 24) == 0


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_the_soft_flags_parse_with_their_partners():
    from diffsim_amd.cli import arg_parse
    a = arg_parse(["--dataset", "cute", "--mask_path", "m", "--soft_masks"])
    assert a.soft_masks is True and a.text_soft is False and a.mask_path == "m" and a.use_mask is True
    b = arg_parse(["--dataset", "nights", "--text_attn", "cat", "--text_soft", "--text_threshold", "0.5"])
    assert b.text_soft is True and b.soft_masks is False and b.text_attn == ["cat"] and b.use_text_attn is True
    assert arg_parse(["--dataset", "nights", "--mask_path", "m", "--soft_masks", "--metric", "diffsim_xl"]).soft_masks is True


@pytest.mark.parametrize("flag,partner", [("--soft_masks", ["--mask_path", "m"]), ("--text_soft", ["--text_attn"])])
def test_the_soft_flags_misused(flag, partner, capsys):
    from diffsim_amd.cli import FEATURE_METRICS, VIT_METRICS, arg_parse
    bad = [[flag], ["--dataset", "cute", flag], ["--dataset", "retrieval", flag] + partner,
           ["--dataset", "cute", "--taps", "up_blocks:0", flag] + partner]
    bad += [["--dataset", "cute", "--metric", m, flag] + partner for m in sorted(VIT_METRICS) + sorted(FEATURE_METRICS)]
    assert len(bad) >= 6
    for argv in bad:
        with pytest.raises(SystemExit) as e:
            arg_parse(argv)
        assert e.value.code == 2, argv
        assert flag in capsys.readouterr().err, argv


def test_accepted_argument_lists_parse_as_before():
    """tests/golden/soft_cli_namespaces.json: the namespaces the argument lists test_region_host.py and test_textattn_host.py accept
    parsed to before the two flags existed."""
    from diffsim_amd.cli import arg_parse
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "soft_cli_namespaces.json")))
    assert len(cases) == 7
    for c in cases:
        got = vars(arg_parse(c["argv"]))
        assert got.pop("soft_masks") is False and got.pop("text_soft") is False
        assert got == c["namespace"], c["argv"]


def test_weight_rows_are_checked_against_the_grid():
    from diffsim_amd.regions import SOFT
    _flat_weights = SOFT.flat_rows
    g = torch.Generator().manual_seed(4)
    w = torch.randint(1, 256, (3, 4, 4), generator=g).to(torch.uint8)
    assert torch.equal(_flat_weights(w, 3, (4, 4), "w"), w.reshape(3, 16)) and torch.equal(_flat_weights(w.reshape(3, 16), 3, (4, 4), "w"),
                                                                                           w.reshape(3, 16))
    w[1] = 0
    with pytest.raises(ValueError, match="image 1 are all 0"):
        _flat_weights(w, 3, (4, 4), "w")
    with pytest.raises(ValueError, match="token grid"):
        _flat_weights(w, 3, (4, 5), "w")
    with pytest.raises(ValueError, match="uint8"):
        _flat_weights(w.float(), 3, (4, 4), "w")
