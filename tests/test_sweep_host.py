"""Tap sweeps on the host: --taps SPEC parsing, the `all` expansion of every model, and the refusals (no GPU needed)."""
import pytest

from diffsim_amd import cli, config as C
from diffsim_amd.sweep import all_taps, parse_tap_specs, tap_label


def test_all_expands_to_every_tap_of_the_addressing():
    sd = all_taps(C.SD15)
    assert sd == [("down_blocks", 0), ("down_blocks", 1), ("down_blocks", 2), ("mid_blocks", 0), ("up_blocks", 0),
                  ("up_blocks", 1), ("up_blocks", 2)]
    xl = all_taps(C.SDXL)
    assert len(xl) == 70
    assert sum(b == "down_blocks" for b, _ in xl) == 24 and sum(b == "mid_blocks" for b, _ in xl) == 10
    assert sum(b == "up_blocks" for b, _ in xl) == 36
    assert ("down_blocks", [1, 1, 9]) in xl and ("mid_blocks", [0, 9]) in xl and ("up_blocks", [1, 2, 1]) in xl
    assert ("up_blocks", [1, 0, 2]) not in xl and ("down_blocks", [0, 0, 2]) not in xl      # depth 2 at SDXL's 640-channel level
    assert len({(b, tuple(l)) for b, l in xl}) == 70
    assert all_taps(C.DIT_XL2) == list(range(28)) and all_taps(C.DIT_TINY) == [0, 1, 2]
    assert len(all_taps(C.TINY)) == 7 and len(all_taps(C.SDXL_TINY)) == 4 + 6 + 3 + 9 + 6
    for metric, cfg, n in (("diffsim", C.SD15, 7), ("diffsim_xl", C.SDXL, 70), ("dit", C.DIT_XL2, 28)):
        assert parse_tap_specs(["all"], metric, cfg) == all_taps(cfg) and len(all_taps(cfg)) == n
        assert parse_tap_specs(["all"], metric) == "all"


def test_spec_forms():
    assert parse_tap_specs(["up_blocks:0", "down_blocks:2", "mid_blocks:0"], "diffsim", C.SD15) == \
        [("up_blocks", 0), ("down_blocks", 2), ("mid_blocks", 0)]
    assert parse_tap_specs(["up_blocks:0,1,9", "mid_blocks:0,5", "down_blocks:1,0,3"], "diffsim_xl", C.SDXL) == \
        [("up_blocks", [0, 1, 9]), ("mid_blocks", [0, 5]), ("down_blocks", [1, 0, 3])]
    assert parse_tap_specs(["blocks:13", "blocks:0"], "dit", C.DIT_XL2) == [13, 0]
    assert tap_label(("up_blocks", 2)) == ("up_blocks", [2]) and tap_label(("mid_blocks", [0, 5])) == ("mid_blocks", [0, 5])


@pytest.mark.parametrize("metric,specs", [
    ("diffsim", ["side_blocks:0"]),                 # unknown block
    ("diffsim", ["up_blocks:0,1,2"]),               # SDXL arity on SD1.5
    ("diffsim", ["up_blocks"]),                     # no index
    ("diffsim", ["up_blocks:x"]),
    ("diffsim", ["up_blocks:1", "up_blocks:1"]),    # duplicate
    ("diffsim", ["all", "up_blocks:1"]),
    ("diffsim_xl", ["up_blocks:0"]),                # SD1.5 arity on SDXL
    ("diffsim_xl", ["mid_blocks:0,1,2"]),
    ("diffsim_xl", ["up_blocks:0,1,9", "up_blocks:0,1,9"]),
    ("dit", ["up_blocks:3"]),
    ("dit", ["blocks:1,2"]),
    ("dit", ["blocks:4", "blocks:4"]),
])
def test_spec_rejections(metric, specs):
    with pytest.raises(ValueError):
        parse_tap_specs(specs, metric)
    with pytest.raises(SystemExit):
        cli.arg_parse(["--metric", metric, "--taps"] + specs)


def test_taps_the_model_does_not_have():
    for metric, cfg, spec in (("diffsim", C.SD15, "up_blocks:3"), ("diffsim", C.SD15, "down_blocks:3"),
                              ("diffsim_xl", C.SDXL, "up_blocks:1,0,2"), ("diffsim_xl", C.SDXL, "mid_blocks:1,0"),
                              ("dit", C.DIT_XL2, "blocks:28")):
        with pytest.raises(ValueError):
            parse_tap_specs([spec], metric, cfg)


def test_cli_accepts_taps_for_the_triplet_datasets_and_refuses_the_rest(tmp_path):
    for ds in ("cute", "nights", "sref"):
        a = cli.arg_parse(["--dataset", ds, "--taps", "up_blocks:0", "mid_blocks:0"])
        assert a.taps == ["up_blocks:0", "mid_blocks:0"]
    assert cli.arg_parse(["--metric", "dit", "--taps", "all"]).taps == ["all"]
    assert cli.arg_parse([]).taps is None
    with pytest.raises(SystemExit):
        cli.arg_parse(["--dataset", "retrieval", "--taps", "up_blocks:0"])
    with pytest.raises(SystemExit):
        cli.arg_parse(["--dataset", "retrieval", "--save_maps", "--taps", "up_blocks:0"])
    with pytest.raises(SystemExit):
        cli.arg_parse(["--save_maps", "--taps", "up_blocks:0"])


def test_cli_taps_all_resolves_against_the_model(tmp_path):
    import types
    for metric, cfg, n in (("diffsim", C.SD15, 7), ("diffsim_xl", C.SDXL, 70), ("dit", C.DIT_XL2, 28), ("diffsim", C.TINY, 7)):
        a = cli.arg_parse(["--metric", metric, "--taps", "all"])
        assert cli.cli_taps(a, types.SimpleNamespace(cfg=cfg)) == all_taps(cfg) and len(all_taps(cfg)) == n
        assert cli.cli_taps(a, None) == all_taps({"diffsim": C.SD15, "diffsim_xl": C.SDXL, "dit": C.DIT_XL2}[metric])
    a = cli.arg_parse(["--metric", "diffsim_xl", "--taps", "up_blocks:1,0,2"])
    with pytest.raises(SystemExit):
        cli.cli_taps(a, None)
