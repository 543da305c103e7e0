"""clip_cross / dino_cross on the host: the float64 restatement (tests/_vit64.py) pinned against transformers' CLIPVisionModel /
Dinov2Model in double and against the reference's own score tails (tests/golden/g11_vit_tails.npz, written by
tests/golden/make_golden_vit.py); the preprocessing against HF's image processors; the HF key maps; the ABI; the CLI."""
import dataclasses
import json
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from diffsim_amd import _lib, config as C, synth as S, vit as V
from tests import _vit64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _hf_model(cfg, sd):
    """transformers' model of cfg in double, loaded with the neutral state dict sd through _vit64's key map"""
    transformers = pytest.importorskip("transformers")
    if cfg.kind == "clip":
        hc = transformers.CLIPVisionConfig(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.depth, num_attention_heads=cfg.num_heads,
                                           intermediate_size=cfg.mlp_dim, patch_size=cfg.patch_size, image_size=cfg.image_size,
                                           layer_norm_eps=cfg.ln_eps, hidden_act="quick_gelu")
        m = transformers.CLIPVisionModel(hc)
        prefix = _hf_prefix(m, "embeddings.class_embedding")
    else:
        hc = transformers.Dinov2Config(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.depth, num_attention_heads=cfg.num_heads,
                                       mlp_ratio=cfg.mlp_dim // cfg.hidden_size, patch_size=cfg.patch_size,
                                       image_size=cfg.pos_grid * cfg.patch_size, layer_norm_eps=cfg.ln_eps, hidden_act="gelu")
        m = transformers.Dinov2Model(hc)
        prefix = _hf_prefix(m, "embeddings.cls_token")
    missing, unexpected = m.load_state_dict(R.to_hf(sd, cfg.kind, cfg.depth, prefix), strict=False)
    assert not unexpected, unexpected
    assert all(("post_layernorm" in k or "mask_token" in k or k.startswith("layernorm.")) for k in missing), missing
    return m.double().eval(), prefix


def _hf_prefix(m, leaf):
    return next(k for k in m.state_dict() if k.endswith(leaf))[: -len(leaf)]


def _pixels(n, side, seed=5):
    return torch.randn(n, 3, side, side, generator=torch.Generator().manual_seed(seed))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("cfg,side", [(C.VIT_TINY_CLIP, 40), (C.VIT_TINY_DINO, 40), (C.VIT_TINY_DINO, 64)],
                         ids=["clip-40", "dinov2-40", "dinov2-64-interpolated"])
def test_vit64_matches_transformers(cfg, side):
    """hidden_states[L] and the hook-equivalent q / k / v (the HF modules' own projections on the hooks' inputs: CLIP the encoder
    layer's raw input, DINOv2 norm1's output) to 1e-10 relative, at every layer; DINOv2 also at a side whose grid differs from the
    stored one (interpolated positions)."""
    sd = S.make_state_dict(cfg, 3)
    m, _ = _hf_model(cfg, sd)
    x = _pixels(2, side)
    with torch.no_grad():
        kw = {"interpolate_pos_encoding": False} if cfg.kind == "clip" else {}
        hs = m(pixel_values=x.double(), output_hidden_states=True, **kw).hidden_states
        mine = R.hidden_states(sd, cfg, x, cfg.depth - 1)
        for L in range(cfg.depth):
            assert _rel(mine[L], hs[L]) < 1e-10, L
            if cfg.kind == "clip":
                a = getattr(m, "vision_model", m).encoder.layers[L].self_attn      # (flat since transformers 5)
                want = a.q_proj(hs[L]), a.k_proj(hs[L]), a.v_proj(hs[L])
            else:
                lay = m.encoder.layer[L]
                a, y = lay.attention.attention, lay.norm1(hs[L])
                want = a.query(y), a.key(y), a.value(y)
            for got, w in zip(R.tap_qkv(sd, cfg, x, L), want):
                assert _rel(got, w) < 1e-10, L


def test_engine_position_table_is_hf_interpolation():
    from diffsim_amd.engine import interpolate_pos_embed
    pos = S.make_state_dict(C.VIT_TINY_DINO, 3, ["pos_embed"])["pos_embed"]
    assert interpolate_pos_embed(pos, 5) is pos
    assert torch.equal(interpolate_pos_embed(pos, 16).double(), R.pos_at(pos, 16))


@pytest.mark.parametrize("kind", ["clip", "dinov2"])
def test_preprocessing_matches_hf_processors(kind):
    """RGB, shortest edge (224 | 256, PIL bicubic), centre crop 224, / 255, mean / std: within 1e-6 of CLIPImageProcessor /
    BitImageProcessor on a golden image and a non-square synthetic one."""
    transformers = pytest.importorskip("transformers")
    if kind == "clip":
        proc = transformers.CLIPImageProcessor(size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224},
                                               image_mean=list(V.CLIP_MEAN), image_std=list(V.CLIP_STD), resample=3)
        mine = V.CLIP_PREPROCESS
    else:
        proc = transformers.BitImageProcessor(size={"shortest_edge": 256}, crop_size={"height": 224, "width": 224},
                                              image_mean=list(V.IMAGENET_MEAN), image_std=list(V.IMAGENET_STD), resample=3)
        mine = V.DINOV2_PREPROCESS
    g = np.random.default_rng(4)
    synth = Image.fromarray((g.random((301, 517, 3)) * 255).astype(np.uint8))
    tall = Image.fromarray((g.random((640, 333, 3)) * 255).astype(np.uint8))
    for im in (Image.open(os.path.join(GOLDEN, "g1_img_c.png")), synth, tall):
        want = torch.as_tensor(np.asarray(proc(images=im.convert("RGB"), return_tensors="np")["pixel_values"]))
        got = mine(im)
        assert got.shape == want.shape == (1, 3, 224, 224) and got.dtype == torch.float32
        assert float((got - want).abs().max()) <= 1e-6


def test_preprocessor_config_overrides_defaults(tmp_path):
    (tmp_path / "preprocessor_config.json").write_text(json.dumps(
        {"size": {"shortest_edge": 48}, "crop_size": {"height": 40, "width": 40}, "image_mean": [0.5, 0.5, 0.5], "image_std": [0.25, 0.5, 1.0]}))
    p = V.Preprocess.from_dir(str(tmp_path), V.DINOV2_PREPROCESS)
    assert (p.resize, p.crop) == (48, 40) and p.std.tolist() == [0.25, 0.5, 1.0]
    assert p(Image.new("RGB", (100, 60), (255, 128, 0))).shape == (1, 3, 40, 40)
    assert V.Preprocess.from_dir(str(tmp_path / "none"), V.CLIP_PREPROCESS) is V.CLIP_PREPROCESS


@pytest.mark.parametrize("cfg,prefixes", [(C.VIT_TINY_CLIP, ("", "vision_model.")), (C.VIT_TINY_DINO, ("", "dinov2."))],
                         ids=["clip", "dinov2"])
def test_hf_key_maps_round_trip(cfg, prefixes):
    """neutral -> HF keys (either prefix form, plus keys the path never reads) -> vit.neutral_state_dict gives the tensors back, and
    agrees with _vit64's own map."""
    sd = S.make_state_dict(cfg, 3)
    for prefix in prefixes:
        hf = R.to_hf(sd, cfg.kind, cfg.depth, prefix)
        hf["text_model.embeddings.token_embedding.weight"] = torch.zeros(3, 4)
        hf[prefix + "post_layernorm.weight"] = torch.zeros(4)
        back = V.neutral_state_dict(hf, cfg)
        assert set(back) == set(sd) == set(C.vit_param_shapes(cfg))
        for k in sd:
            assert back[k].shape == sd[k].shape and torch.equal(back[k], sd[k]), k
        mine = R.to_neutral(hf, cfg.kind, cfg.depth, prefix)
        assert all(torch.equal(mine[k], sd[k]) for k in sd)


def test_config_from_hf_json():
    c = V.vit_config_from_json({"vision_config": {"hidden_size": 128, "num_hidden_layers": 3, "num_attention_heads": 2,
                                                  "intermediate_size": 256, "patch_size": 8, "image_size": 40}}, "clip")
    assert c == C.VIT_TINY_CLIP
    d = V.vit_config_from_json({"hidden_size": 128, "num_hidden_layers": 3, "num_attention_heads": 2, "mlp_ratio": 4, "patch_size": 8,
                                "image_size": 40, "layer_norm_eps": 1e-6}, "dinov2")
    assert dataclasses.replace(d, image_size=40) == C.VIT_TINY_DINO
    assert V.vit_config_from_json({}, "clip") == C.CLIP_B32 and V.vit_config_from_json({}, "dinov2") == C.DINOV2_S14
    with pytest.raises(ValueError, match="SwiGLU"):
        V.vit_config_from_json({"use_swiglu_ffn": True}, "dinov2")


def test_tails_match_the_reference_capture():
    """_vit64's tails on the q / k / v the reference's own attention_calc ran on (make_golden_vit.py), within 1e-6."""
    z = np.load(os.path.join(GOLDEN, "g11_vit_tails.npz"))
    q, k, v = (torch.from_numpy(z[n]) for n in "qkv")              # (2, H, N, D)
    H = q.shape[1]
    flat = lambda t: t.transpose(1, 2).reshape(2, 1, t.shape[2], -1)      # [n_feat][B = 1][N][H*D]
    q, k, v = flat(q), flat(k), flat(v)
    w, b = torch.from_numpy(z["w_out"]), torch.from_numpy(z["bias"])
    dino = R.pair_scores(q, k, v, [0], [1], H)
    clip = R.pair_scores(q, k, v, [0], [1], H, "cosine", w, b)
    assert abs(float(dino[0]) - float(z["dino_cross"][0])) < 1e-6
    assert abs(float(clip[0]) - float(z["clip_cross"][0])) < 1e-6
    assert abs(float(clip[0]) - float(dino[0])) > 1e-3          # the projection matters on this capture


def test_header_declares_and_lib_binds_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    names = ["dsim_vit_create", "dsim_vit_destroy", "dsim_vit_load_weight", "dsim_vit_finalize", "dsim_vit_set_tap",
             "dsim_vit_workspace_bytes", "dsim_vit_qkv", "dsim_vit_taps_workspace_bytes", "dsim_vit_qkv_taps", "dsim_vit_profile",
             "dsim_vit_profile_count", "dsim_vit_profile_get", "dsim_pair_score_proj", "dsim_pair_score_proj_workspace_bytes"]
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert n in _lib.SYMBOLS, n
    assert int(re.search(r"#define\s+DSIM_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION == 7
    L = _lib.lib()                                  # binds every declared symbol or raises
    assert L.dsim_version() == 7
    # the cfg struct mirrors the header's field order
    fields = re.search(r"typedef struct dsim_vit_cfg \{(.*?)\} dsim_vit_cfg;", header, re.S).group(1)
    assert re.findall(r"(?:int32_t|float)\s+(\w+);", fields) == [f[0] for f in _lib.ViTCfgC._fields_]
    # host-side refusals of the projected tail's workspace query (nothing touches a device)
    q = L.dsim_pair_score_proj_workspace_bytes
    assert q(1, 1, 2, 26, 64, _lib.DSIM_BF16) > 0
    for bad in ((0, 1, 2, 26, 64, 1), (32768, 1, 2, 26, 64, 1), (1, 1, 2, 26, 48, 1), (1, 1, 2, 26, 64, 7), (1, 1, 32, 26, 64, 0)):
        assert q(*bad) == 0, bad


def _write_checkpoint(folder, cfg, prefix=""):
    from safetensors.torch import save_file
    os.makedirs(folder, exist_ok=True)
    sd = S.make_state_dict(cfg, 3)
    save_file(R.to_hf(sd, cfg.kind, cfg.depth, prefix), os.path.join(folder, "model.safetensors"))
    if cfg.kind == "clip":
        j = {"vision_config": {"hidden_size": cfg.hidden_size, "num_hidden_layers": cfg.depth, "num_attention_heads": cfg.num_heads,
                               "intermediate_size": cfg.mlp_dim, "patch_size": cfg.patch_size, "image_size": cfg.image_size}}
    else:
        j = {"hidden_size": cfg.hidden_size, "num_hidden_layers": cfg.depth, "num_attention_heads": cfg.num_heads,
             "mlp_ratio": cfg.mlp_dim // cfg.hidden_size, "patch_size": cfg.patch_size, "image_size": cfg.pos_grid * cfg.patch_size}
    with open(os.path.join(folder, "config.json"), "w") as f:
        json.dump(j, f)
    with open(os.path.join(folder, "preprocessor_config.json"), "w") as f:
        json.dump({"size": {"shortest_edge": 48}, "crop_size": {"height": cfg.image_size, "width": cfg.image_size}}, f)
    return sd


@pytest.mark.parametrize("metric,cfg", [("dino_cross", C.VIT_TINY_DINO), ("clip_cross", C.VIT_TINY_CLIP)])
def test_cli_reaches_the_engine(metric, cfg, tmp_path, monkeypatch):
    """--metric dino_cross / clip_cross on a tiny checkpoint directory: config, weights and preprocessor load on the host and the
    run stops where the engine needs the GPU (DsimError), not at build_scorer's "out of scope" SystemExit."""
    from diffsim_amd import cli
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    _write_checkpoint(str(tmp_path / "ckpt"), cfg, "vision_model." if metric == "clip_cross" else "")
    (tmp_path / "images").mkdir()
    with pytest.raises(_lib.DsimError, match="no GPU"):
        cli.main(["--metric", metric, "--dataset", "cute", "--model_path", str(tmp_path / "ckpt"), "--image_path",
                  str(tmp_path / "images"), "--target_layer", "1"])


def test_cli_refusals(tmp_path, capsys):
    from diffsim_amd import cli
    with pytest.raises(SystemExit, match="out of scope"):
        cli.main(["--metric", "clip_i", "--dataset", "cute", "--model_path", str(tmp_path), "--image_path", str(tmp_path)])
    base = ["--model_path", str(tmp_path), "--image_path", str(tmp_path)]
    cases = [(["--metric", "clip_cross", "--dataset", "retrieval", "--query_path", "q", "--out_path", "o"], "no projected score matrix"),
             (["--metric", "dino_cross", "--dataset", "cute", "--mask_path", "m"], "--mask_path"),
             (["--metric", "clip_cross", "--dataset", "cute", "--text_attn"], "--text_attn"),
             (["--metric", "dino_cross", "--dataset", "retrieval", "--query_path", "q", "--out_path", "o", "--save_maps"], "--save_maps"),
             (["--metric", "dino_cross", "--dataset", "retrieval", "--query_path", "q", "--out_path", "o", "--save_matches"], "--save_matches"),
             (["--metric", "clip_cross", "--dataset", "cute", "--fp8_attention"], "--fp8_attention")]
    for extra, text in cases:
        with pytest.raises(SystemExit) as e:
            cli.arg_parse(base + extra)
        assert e.value.code == 2
        assert text in capsys.readouterr().err, extra
    ok = cli.arg_parse(base + ["--metric", "dino_cross", "--dataset", "cute", "--taps", "layers:0", "layers:2"])
    assert cli.cli_taps(ok, None) == [0, 2]
    with pytest.raises(SystemExit):
        cli.arg_parse(base + ["--metric", "clip_cross", "--dataset", "cute", "--taps", "blocks:1"])


def test_scorer_protocol_defaults_are_todays_behaviour():
    """The three facts the ViT kinds override, at their defaults: process_image in front of the VAE, draws, the plain pair tail."""
    from diffsim_amd.image import load_image, process_image
    from diffsim_amd.scorer import Scorer
    s = Scorer()
    im = Image.open(os.path.join(GOLDEN, "g1_img_c.png"))
    assert torch.equal(s.load_input(im, 64), process_image(load_image(im), 64))
    assert s.draws is True and s.pair_tail(("up_blocks", 0)) is None
    assert V.CLIPScore.draws is False and V.Dinov2Score.draws is False
    assert V.Dinov2Score.pair_tail is Scorer.pair_tail and V.CLIPScore.pair_tail is not Scorer.pair_tail


def test_path_latents_of_a_drawless_kind_are_its_preprocessed_pixels():
    from diffsim_amd.inputs import path_latents
    pre = V.Preprocess(48, 40, V.IMAGENET_MEAN, V.IMAGENET_STD)
    sc = V.Dinov2Score(C.VIT_TINY_DINO, {}, "cuda", torch.float32, pre)        # (no engine is made until features are asked for)
    a, b = os.path.join(GOLDEN, "g1_img_a.png"), os.path.join(GOLDEN, "g1_img_b.png")
    (ca, cb), nA, nB = path_latents(sc, [(a, b), (b, a)], (0, 1), 512, 2334, 16)
    assert ca.shape == cb.shape == (2, 3, 40, 40) and nA.shape == (1, 3, 40, 40) and not nA.any() and not nB.any()
    assert torch.equal(ca[0], pre(Image.open(a))[0]) and torch.equal(cb[0], ca[1]) and torch.equal(ca[1], pre(Image.open(b))[0])
