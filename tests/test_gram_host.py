"""The gram metric without a GPU: the ABI of the new entry points, the float64 restatement tests/_gram64.py against the golden captured
from the reference's own code (tests/golden/make_golden_gram.py -> g13_gram.npz), the resize rule against PIL, the key map and plan
parsing, the loader's files, and the command line's acceptance and refusals."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from diffsim_amd import _lib, gram as G
from tests import _gram64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g13_gram.npz")
NEW = {"dsim_vgg_create": 2, "dsim_vgg_destroy": 1, "dsim_vgg_load_weight": 6, "dsim_vgg_finalize": 2, "dsim_vgg_profile": 2,
       "dsim_vgg_profile_count": 1, "dsim_vgg_profile_get": 7, "dsim_vgg_out_shape": 6, "dsim_vgg_workspace_bytes": 4,
       "dsim_vgg_features": 9, "dsim_op_relu": 4, "dsim_op_relu_pool2": 8, "dsim_gram_rows_workspace_bytes": 6, "dsim_gram_rows": 12,
       "dsim_feature_matrix_chunked_workspace_bytes": 5, "dsim_feature_matrix_chunked": 14}


def test_header_declares_and_lib_exports_the_symbols():
    text = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+DSIM_ABI_VERSION\s+7\b", header) and _lib.ABI_VERSION == 7            # additive: the version stays
    L = _lib.lib()
    for name, nargs in NEW.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header, re.S)
        assert m, f"{name} is not declared"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SYMBOLS[name][1]), name
        assert hasattr(L, name), name
    assert re.search(r"#define\s+DSIM_VGG_MAX_PLAN\s+%d\b" % _lib.VGG_MAX_PLAN, header)
    assert "LAST ROW" in open(os.path.join(ROOT, "diffsim_amd", "gram.py")).read() and "conv5_1" in text


def test_gram_rows_workspace_query_refuses_on_the_host():
    q = _lib.lib().dsim_gram_rows_workspace_bytes
    assert q(3, 1024, 512, 0, 512, _lib.DSIM_BF16) >= 3 * 2 * 512 * 512 * 4          # two partials per image at P = 1024
    assert q(3, 108, 256, 255, 1, _lib.DSIM_F32) >= 3 * 256 * 4
    for bad in ((0, 10, 64, 0, 64, 1), (2, 0, 64, 0, 64, 1), (2, 10, 60, 0, 60, 1), (2, 10, 64, 0, 65, 1), (2, 10, 64, 64, 1, 1),
                (2, 10, 64, -1, 1, 1), (2, 10, 64, 0, 0, 1), (2, 10, 64, 0, 64, 7), (65536, 10, 64, 0, 64, 1), (2, 10, 0, 0, 0, 1)):
        assert q(*bad) == 0, bad


def test_chunked_matrix_workspace_query():
    L = _lib.lib()
    q, q0 = L.dsim_feature_matrix_chunked_workspace_bytes, L.dsim_feature_matrix_workspace_bytes
    assert q(3, 5, 65536, _lib.DSIM_F32, 16384) == q0(3, 5, 65536, _lib.DSIM_F32) > 0          # the default chunk: the plain call's
    assert q(3, 5, 65536, _lib.DSIM_F32, 1024) >= 64 * 15 * 4                                  # 64 partials per cell
    for bad in ((3, 5, 65536, 0, 1000), (3, 5, 65536, 0, 32), (3, 5, 65536, 0, 32768), (3, 5, 65536, 0, 0), (3, 5, 65536, 9, 1024),
                (0, 5, 65536, 0, 1024), (3, 5, 65532, 0, 1024), (2, 2, 1 << 30, 0, 64)):
        assert q(*bad) == 0, bad


# ---- the restatement against the reference's own numbers --------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_golden():
    """gram_matrix and line 81, run by the reference itself on float64 features: the restatement agrees at 1e-10; on these inputs the
    last-row cosine (the reference's) and the whole-matrix cosine differ by more than 1e-3."""
    g = np.load(GOLDEN)
    fa, fb = torch.from_numpy(g["feats_a"]), torch.from_numpy(g["feats_b"])
    assert fa.shape == (1, 32, 5, 7) and fa.dtype == torch.float64 and g["gram"].shape == (1,)
    ga, gb = R.gram_matrix(fa), R.gram_matrix(fb)
    assert ga.shape == (32, 32)
    scale = float(ga.abs().max())
    assert float((ga - torch.from_numpy(g["gram_a"])).abs().max()) <= 1e-10 * scale
    assert float((gb - torch.from_numpy(g["gram_b"])).abs().max()) <= 1e-10 * scale
    last, full = float(R.score(ga, gb)), float(R.score(ga, gb, full=True))
    assert abs(last - float(g["gram"][0])) <= 1e-10
    assert abs(float(R.similarity_of_features(fa, fb)) - float(g["gram"][0])) <= 1e-10
    assert abs(full - float(F.cosine_similarity(ga.reshape(1, -1), gb.reshape(1, -1)))) <= 1e-10
    assert abs(last - full) > 1e-3, (last, full)             # the quirk is visible on these inputs


def test_restated_stack_is_torchvisions_layout():
    assert R.conv_indices(R.VGG19_PLAN) == G.conv_indices(G.VGG19_PLAN) == [0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28]
    assert R.VGG19_PLAN == G.VGG19_PLAN and [e for e in G.VGG19_PLAN if e != "P"] == [64, 64, 128, 128] + [256] * 4 + [512] * 5
    sd = R.he_state_dict(R.SMALL_PLAN, seed=1)
    assert sorted(sd) == sorted(f"features.{i}.{leaf}" for i in (0, 2, 5, 7, 10) for leaf in ("weight", "bias"))
    x = torch.randn(1, 3, 37, 51, generator=torch.Generator().manual_seed(2))
    y = R.features(x, sd, R.SMALL_PLAN)
    assert y.shape == (1, 256, 9, 12) and y.dtype == torch.float64 and bool((y < 0).any())        # floor-mode pools; no ReLU on the tap
    # module by module, as the reference runs torchvision's Sequential
    mods, cin = [], 3
    for e in R.SMALL_PLAN:
        if e == "P":
            mods.append(torch.nn.MaxPool2d(2, 2))
        else:
            mods += [torch.nn.Conv2d(cin, e, 3, padding=1), torch.nn.ReLU()]
            cin = e
    seq = torch.nn.Sequential(*mods).double()
    seq.load_state_dict({k[len("features."):]: v.double() for k, v in sd.items()})
    z = x.double()
    for name, layer in seq._modules.items():
        z = layer(z)
        if name == "10":
            break
    assert torch.equal(z, y)


# ---- preprocessing -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,want", [(100, 75, (85, 64)), (75, 100, (64, 85)), (64, 200, (64, 200))])
def test_resize_rule_agrees_with_pil(w, h, want):
    rng = np.random.default_rng(w)
    im = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    assert G.resized_size(w, h, 64) == (want if (w, h) != (64, 200) else (64, 200))
    out = G.resize_image(im, 64)
    assert out.size == want
    if (w, h) == (64, 200):
        assert out is im                                     # short side already 64: returned as it is
    else:
        assert np.array_equal(np.asarray(out), np.asarray(im.resize(want, Image.BILINEAR)))


# ---- key map, plan, loader ---------------------------------------------------------------------------------------------------------------
def test_key_map_and_plan_parsing():
    sd = R.he_state_dict(R.SMALL_PLAN, seed=3)
    n = G.neutral_state_dict(sd, R.SMALL_PLAN)
    assert sorted(n) == sorted(f"convs.{i}.{leaf}" for i in range(5) for leaf in ("weight", "bias"))
    assert n["convs.2.weight"] is sd["features.5.weight"] and n["convs.4.bias"] is sd["features.10.bias"]
    pre = {"vgg." + k: v for k, v in sd.items()}
    pre["vgg.classifier.0.weight"] = torch.zeros(4, 4)
    assert G.neutral_state_dict(pre, R.SMALL_PLAN)["convs.1.weight"] is sd["features.2.weight"]
    with pytest.raises(ValueError, match="features.5.weight"):
        G.neutral_state_dict({k: v for k, v in sd.items() if k != "features.5.weight"}, R.SMALL_PLAN)
    with pytest.raises(ValueError, match="plan's conv 1"):
        G.neutral_state_dict(sd, (64, 128, "P", 128, 128, "P", 256))
    assert G.parse_plan([64, 64, "M", 128, 0, 256]) == (64, 64, "P", 128, "P", 256)
    for bad in (["P", 64], [64, "P"], [64, "P", "P", 64], [12], [64, -8, 64], [64, 1.5], [], [True]):
        with pytest.raises(ValueError):
            G.parse_plan(bad)


def _write_checkpoint(folder, plan=R.SMALL_PLAN, seed=4, pth=False):
    os.makedirs(folder, exist_ok=True)
    sd = R.he_state_dict(plan, seed=seed)
    if pth:
        torch.save(sd, os.path.join(folder, "vgg.pth"))
    else:
        from safetensors.torch import save_file
        save_file(sd, os.path.join(folder, "model.safetensors"))
    with open(os.path.join(folder, "config.json"), "w") as f:
        json.dump({"plan": list(plan)}, f)
    return sd


@pytest.mark.parametrize("pth", [False, True], ids=["safetensors", "pth"])
def test_loader_reads_both_file_kinds(tmp_path, pth):
    from diffsim_amd import loader
    sd = _write_checkpoint(str(tmp_path), pth=pth)
    plan, got = loader.vgg_gram_files(str(tmp_path))
    assert plan == R.SMALL_PLAN and sorted(got) == sorted(sd) and torch.equal(got["features.7.weight"], sd["features.7.weight"])
    if pth:
        plan2, got2 = loader.vgg_gram_files(str(tmp_path / "vgg.pth"))
        assert plan2 == R.SMALL_PLAN and sorted(got2) == sorted(sd)
    os.remove(str(tmp_path / "config.json"))
    assert loader.vgg_gram_files(str(tmp_path))[0] == G.VGG19_PLAN
    with open(str(tmp_path / "config.json"), "w") as f:
        json.dump({"plan": [64, "P", "P", 64]}, f)
    with pytest.raises(ValueError, match="config.json"):
        loader.vgg_gram_files(str(tmp_path))


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def _base(tmp_path):
    return ["--model_path", str(tmp_path), "--image_path", str(tmp_path), "--metric", "gram"]


def test_cli_accepts_gram_on_every_dataset(tmp_path):
    from diffsim_amd import cli
    assert "gram" in cli.ENGINE_METRICS
    for ds in ("cute", "nights", "sref"):
        a = cli.arg_parse(_base(tmp_path) + ["--dataset", ds, "--similarity", "cosine"])
        assert a.metric == "gram" and a.gram_full is False and "gram_full" not in vars(a)
    a = cli.arg_parse(_base(tmp_path) + ["--dataset", "retrieval", "--query_path", "q", "--out_path", "o", "--similarity", "cosine", "--gram_full"])
    assert a.gram_full is True
    assert cli.arg_parse(_base(tmp_path) + ["--similarity", "cosine", "--ngpu", "1"]).ngpu == 1


def test_cli_refusals(tmp_path, capsys):
    from diffsim_amd import cli
    retr = ["--dataset", "retrieval", "--query_path", "q", "--out_path", "o"]
    cos = ["--similarity", "cosine"]
    cases = [([], "--similarity cosine"), (["--similarity", "mse"], "--similarity cosine"),
             (cos + ["--mask_path", "m"], "--mask_path"), (cos + ["--text_attn"], "--text_attn"),
             (cos + ["--fp8_attention"], "--fp8_attention"), (cos + ["--taps", "all"], "--taps"),
             (cos + ["--ngpu", "2"], "single-GPU"),
             (cos + ["--mask_path", "m", "--transfer_masks"], "--mask_path"),
             (cos + ["--query_mask_path", "m"] + retr, "--query_mask_path"),
             (cos + ["--gallery_mask_path", "m"] + retr, "--gallery_mask_path"),
             (cos + ["--query_mask_path", "m", "--transfer_masks"] + retr, "--query_mask_path"),
             (cos + ["--save_maps"] + retr, "--save_maps"), (cos + ["--save_matches"] + retr, "--save_matches"),
             (cos + ["--save_region_maps"] + retr, "--save_region_maps"),
             (cos + ["--save_region_matches"] + retr, "--save_region_matches")]
    for extra, text in cases:
        with pytest.raises(SystemExit) as e:
            cli.arg_parse(_base(tmp_path) + extra)
        err = capsys.readouterr().err
        assert e.value.code == 2 and text in err and "gram" in err, (extra, err)
    with pytest.raises(SystemExit):
        cli.arg_parse(["--metric", "diffsim", "--gram_full", "--model_path", "x", "--image_path", "y"])
    assert "--metric gram" in capsys.readouterr().err


def test_cli_gram_reaches_the_engine_and_clip_i_stays_out_of_scope(tmp_path, monkeypatch, capsys):
    """--metric gram on a tiny checkpoint: the plan and the weights load on the host and the run stops where the engine needs the GPU
    (DsimError), not at build_scorer's "out of scope" exit, which clip_i still takes, word for word."""
    from diffsim_amd import cli
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    _write_checkpoint(str(tmp_path / "ckpt"))
    (tmp_path / "images").mkdir()
    args = ["--dataset", "sref", "--model_path", str(tmp_path / "ckpt"), "--image_path", str(tmp_path / "images"), "--similarity", "cosine"]
    with pytest.raises(_lib.DsimError, match="no GPU"):
        cli.main(["--metric", "gram"] + args)
    assert "last rows of the Gram matrices" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        cli.main(["--metric", "clip_i"] + args)
    assert str(e.value) == ("--metric clip_i: only the DiffSim metrics (diffsim, diffsim_xl, dit, clip_cross, dino_cross) run on this engine; "
                            "the competitor metrics of the reference are out of scope")
