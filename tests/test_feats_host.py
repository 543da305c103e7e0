"""diffeats / dinofeats without a GPU: the ABI of the three entry points and their workspace queries, the command line's acceptance and
refusals, the FeatureView protocol (diffsim_amd/feats.py), and the float64 restatement tests/_feats64.py against plain torch."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from diffsim_amd import _lib, config as C
from tests import _feats64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dsim_attn_features": 18, "dsim_attn_features_workspace_bytes": 8, "dsim_feature_pair_score": 12,
       "dsim_feature_pair_score_workspace_bytes": 3, "dsim_feature_matrix": 13, "dsim_feature_matrix_workspace_bytes": 4}


def test_header_declares_and_lib_exports_the_symbols():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "diffsim_amd.h")).read(), flags=re.S)
    assert re.search(r"#define\s+DSIM_ABI_VERSION\s+7\b", header) and _lib.ABI_VERSION == 7            # additive: the version stays
    L = _lib.lib()
    for name, nargs in NEW.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header, re.S)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    assert "NOT bit-equal" in text and "diffeats" in text and "dinofeats" in text


def test_workspace_queries_refuse_on_the_host():
    L = _lib.lib()
    qf, qp, qm = L.dsim_attn_features_workspace_bytes, L.dsim_feature_pair_score_workspace_bytes, L.dsim_feature_matrix_workspace_bytes
    n, B, H, N, D = 2, 2, 8, 130, 160
    Lc = B * N * H * D
    plain, proj = qf(n, B, H, N, D, Lc, _lib.DSIM_BF16, 0), qf(n, B, H, N, D, Lc, _lib.DSIM_BF16, 1)
    assert 0 < plain and proj >= plain + n * Lc * 2                  # the projection keeps the attention outputs in the workspace
    assert qf(n, B, H, N, D, Lc, _lib.DSIM_F32, 1) >= plain + n * Lc * 4
    for bad in ((n, B, H, N, D, Lc, 7, 0), (n, B, H, N, 48, B * N * H * 48, 1, 0), (0, B, H, N, D, Lc, 1, 0), (-1, B, H, N, D, Lc, 1, 0),
                (n, B, H, N, D, Lc + 8, 1, 0), (n, B, H, N, D, Lc - 8, 1, 1), (65536, B, H, N, D, Lc, 1, 0), (n, 8192, 8, 1, 16, 8192 * 128, 1, 0)):
        assert qf(*bad) == 0, bad
    assert qp(7, Lc, _lib.DSIM_F16) > 0 and qm(33, 34, 560, _lib.DSIM_BF16) > 0
    assert qm(2, 3, 332800, _lib.DSIM_F32) >= 21 * 6 * 4            # ceil(332800 / 16384) split-K partials per cell
    for bad in ((0, Lc, 1), (7, Lc, 7), (7, 0, 1), (7, 12, 1), (65536, Lc, 1)):
        assert qp(*bad) == 0, bad
    for bad in ((0, 3, 560, 1), (3, 0, 560, 1), (3, 5, 560, 9), (3, 5, 564, 1), (3, 5, 0, 1), (65536, 65536, 560, 1)):
        assert qm(*bad) == 0, bad


def _base(tmp_path):
    return ["--model_path", str(tmp_path), "--image_path", str(tmp_path)]


@pytest.mark.parametrize("metric", ["diffeats", "dinofeats"])
def test_cli_parses_both_metrics_and_refuses_what_they_do_not_have(metric, tmp_path, capsys):
    from diffsim_amd import cli
    base = _base(tmp_path) + ["--metric", metric]
    for ds in ("cute", "nights", "sref"):
        a = cli.arg_parse(base + ["--dataset", ds, "--similarity", "cosine"])
        assert a.metric == metric and metric in cli.ENGINE_METRICS
    cli.arg_parse(base + ["--dataset", "retrieval", "--query_path", "q", "--out_path", "o", "--similarity", "cosine"])
    spec = "up_blocks:1" if metric == "diffeats" else "layers:1"
    a = cli.arg_parse(base + ["--dataset", "cute", "--similarity", "cosine", "--taps", spec])
    assert cli.cli_taps(a, None) == ([("up_blocks", 1)] if metric == "diffeats" else [1])
    retr = ["--dataset", "retrieval", "--query_path", "q", "--out_path", "o"]
    cases = [([], "--similarity cosine"), (["--similarity", "mse"], "--similarity cosine"),
             (["--similarity", "cosine", "--mask_path", "m"], "--mask_path"),
             (["--similarity", "cosine", "--text_attn"], "--text_attn"),
             (["--similarity", "cosine", "--fp8_attention"], "--fp8_attention"),
             (["--similarity", "cosine", "--query_mask_path", "m"] + retr, "--query_mask_path"),
             (["--similarity", "cosine", "--gallery_mask_path", "m"] + retr, "--gallery_mask_path"),
             (["--similarity", "cosine", "--save_maps"] + retr, "--save_maps"),
             (["--similarity", "cosine", "--save_matches"] + retr, "--save_matches"),
             (["--similarity", "cosine", "--save_region_maps"] + retr, "--save_region_maps"),
             (["--similarity", "cosine", "--save_region_matches"] + retr, "--save_region_matches")]
    for extra, text in cases:
        with pytest.raises(SystemExit) as e:
            cli.arg_parse(base + extra)
        err = capsys.readouterr().err
        assert e.value.code == 2 and text in err and metric in err, (extra, err)


def test_cli_diffeats_reaches_the_engine_and_clipfeats_stays_out_of_scope(tmp_path):
    """--metric diffeats on a tiny SD1.5 checkpoint: configs and weights load on the host and the run stops where the engine needs
    the GPU (DsimError), not at build_scorer's "out of scope" exit; clipfeats still takes that exit, and so does --ip_adapter."""
    from diffsim_amd import cli
    from tests.test_cli import _write_checkpoint
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    ck = str(tmp_path / "ckpt")
    os.makedirs(ck)
    _write_checkpoint(ck)
    (tmp_path / "images").mkdir()
    args = ["--dataset", "cute", "--model_path", ck, "--image_path", str(tmp_path / "images"), "--target_layer", "1", "--similarity", "cosine"]
    with pytest.raises(_lib.DsimError, match="no GPU"):
        cli.main(["--metric", "diffeats"] + args)
    with pytest.raises(SystemExit, match="out of scope"):
        cli.main(["--metric", "clipfeats"] + args)
    with pytest.raises(SystemExit, match="out of scope"):
        cli.main(["--metric", "diffeats", "--ip_adapter"] + args)


def test_cli_dinofeats_reaches_the_engine(tmp_path, monkeypatch, capsys):
    from diffsim_amd import cli
    from tests.test_vit_host import _write_checkpoint
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    _write_checkpoint(str(tmp_path / "ckpt"), C.VIT_TINY_DINO)
    (tmp_path / "images").mkdir()
    with pytest.raises(_lib.DsimError, match="no GPU"):
        cli.main(["--metric", "dinofeats", "--dataset", "cute", "--model_path", str(tmp_path / "ckpt"), "--image_path",
                  str(tmp_path / "images"), "--target_layer", "1", "--similarity", "cosine"])
    assert "--image_size is not consulted" in capsys.readouterr().out


def test_feature_view_protocol():
    from diffsim_amd import feats, vit as V
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.diffsim_dit import diffsim_DiT
    from diffsim_amd.diffsim_xl import diffsim_xl
    from diffsim_amd.scorer import Scorer
    assert Scorer().matrix_tail(("up_blocks", 0)) is None and Scorer().pair_tail(("up_blocks", 0)) is None
    ds = DiffSim.__new__(DiffSim)           # (the tap rule reads no state)
    view = feats.FeatureView(ds)
    assert ds.tap_of("up_blocks", [2]) == ("up_blocks", 0)                     # DiffSim.diffsim forces a single value to 0 ...
    assert view.tap_of("up_blocks", [2]) == ("up_blocks", 2)                   # ... diffeats takes it literally (diffeats.py:143-144)
    assert view.tap_of("mid_blocks", 0) == ("mid_blocks", 0)
    with pytest.raises(ValueError):
        view.tap_of("up_blocks", [1, 2])
    assert view.metric == "diffeats" and view.draws is True                    # everything else is the wrapped scorer's
    dino = V.Dinov2Score(C.VIT_TINY_DINO, {}, "cuda", torch.float32)
    dv = feats.FeatureView(dino)
    assert dv.metric == "dinofeats" and dv.tap_of(None, [2]) == 2 and dv.draws is False and dv.spec(2) == {"minmax": False}
    assert callable(dv.pair_tail(2)) and dv.matrix_tail(2) is not None and dino.matrix_tail(2) is None
    clip = V.CLIPScore(C.VIT_TINY_CLIP, {}, "cuda", torch.float32)
    assert clip.matrix_tail(1) is None                                         # (retrieval keeps refusing its projected tail)
    for other, name in ((clip, "clipfeats"), (diffsim_xl.__new__(diffsim_xl), "diffeats"), (diffsim_DiT.__new__(diffsim_DiT), "diffeats")):
        with pytest.raises(NotImplementedError, match=name):
            feats.FeatureView(other)
    # the tapped attn1 of every SD1.5 tap: blocks as diffeats.py:156-171 lists them, attentions[-1].transformer_blocks[-1]
    keys = C.unet_param_shapes(C.SD15)
    want = {("down_blocks", 0): ("down_blocks.0.attentions.1.", 320), ("down_blocks", 2): ("down_blocks.2.attentions.1.", 1280),
            ("mid_blocks", 0): ("mid_block.attentions.0.", 1280), ("up_blocks", 0): ("up_blocks.1.attentions.2.", 1280),
            ("up_blocks", 1): ("up_blocks.2.attentions.2.", 640), ("up_blocks", 2): ("up_blocks.3.attentions.2.", 320)}
    for tap, (prefix, c) in want.items():
        p = feats.unet_tap_attention(C.SD15, tap)
        assert p == prefix + "transformer_blocks.0.attn1." and keys[p + "to_out.0.weight"] == (c, c), tap


def test_restatement_against_the_reference_capture():
    """tests/golden/g12_feats.npz (make_golden_feats.py): the reference's own min_max_normalize on seeded features and the cosine
    of diffeats.py:205; the restatement reproduces both at 1e-6."""
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", "g12_feats.npz"))
    norm = {}
    for side in "ab":
        f = torch.from_numpy(z[f"feats_{side}"])
        assert f.shape == (2, 9, 32)
        norm[side], mn, mx = R.min_max_normalize64(f.double(), torch.float32)
        assert mn == float(f.min()) and mx == float(f.max())
        assert float((norm[side] - torch.from_numpy(z[f"norm_{side}"]).double()).abs().max()) <= 1e-6
    assert z["diffeats"].shape == (1,) and abs(R.cosine64(norm["a"], norm["b"]) - float(z["diffeats"][0])) <= 1e-6


def test_restatement_against_plain_torch():
    """tests/_feats64.py on float64 inputs against torch's own SDPA, linear and cosine_similarity, and the reference's
    min_max_normalize written out (metrics/diffeats.py:136-140)."""
    g = torch.Generator().manual_seed(3)
    n, B, H, N, D = 2, 2, 2, 9, 16
    q, k, v = (torch.randn(n, B, N, H * D, generator=g, dtype=torch.float64) for _ in range(3))
    w, b = torch.randn(H * D, H * D, generator=g, dtype=torch.float64) / 6, torch.randn(H * D, generator=g, dtype=torch.float64)
    hd = lambda t: t.view(n * B, N, H, D).transpose(1, 2)
    o = F.scaled_dot_product_attention(hd(q), hd(k), hd(v)).transpose(1, 2).reshape(n, B, N, H * D)
    plain, st = R.features64(q, k, v, H, torch.float64)
    assert (plain - o).abs().max() < 1e-12 and abs(float(st[1, 1]) - float(o[1].min())) < 1e-12
    f = F.linear(o, w, b)
    norm = torch.stack([(x - x.min()) / (x.max() - x.min()) for x in f])
    got, st = R.features64(q, k, v, H, torch.float64, w, b, True)
    assert (got - norm.float().double()).abs().max() < 1e-12
    assert abs(float(st[0, 0]) - float((got[0] ** 2).sum())) < 1e-9 and abs(float(st[0, 2]) - float(f[0].max())) < 1e-12
    want = F.cosine_similarity(got[0].reshape(1, -1), got[1].reshape(1, -1))
    assert abs(R.cosine64(got[0], got[1]) - float(want)) < 1e-12 and abs(float(R.matrix64(got, got)[0, 1]) - float(want)) < 1e-12
    for dtype in (torch.bfloat16, torch.float16, torch.float32):           # the yardstick runs in every pipeline dtype on the CPU
        r = R.restate(q.to(dtype), k.to(dtype), v.to(dtype), H, w.to(dtype), b.float(), True)
        assert r.dtype == dtype and r.shape == (n, B, N, H * D) and float((r.double() - norm).abs().max()) < 0.1
