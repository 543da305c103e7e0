"""Exemplar-guided retrieval, the parts that need no GPU: the command line's accept and refuse cases, the refusals of
retrieval.score_latent_matrix_exemplar / score_path_matrix(exemplar=) that must come before any engine call, the region rule on a matrix's (cells, N) masses
against a loop over transfer.region_of_mass per row, the guide's accounting, and _lib's declarations against the header."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = ["--dataset", "retrieval", "--query_mask_path", "q", "--transfer_masks"]


# ---- the command line
@pytest.mark.parametrize("extra", [[], ["--transfer_threshold", "0.5"], ["--soft_masks"], ["--save_transfer"], ["--metric", "diffsim_xl"],
                                   ["--metric", "dit"], ["--soft_masks", "--save_transfer", "--transfer_threshold", "0"]])
def test_the_flags_are_accepted_with_their_partners(extra):
    from diffsim_amd.cli import arg_parse
    args = arg_parse(GOOD + extra)
    assert args.transfer_masks is True and args.query_mask_path == "q" and args.mask_path is None
    assert args.save_transfer is ("--save_transfer" in extra) and args.soft_masks is ("--soft_masks" in extra)
    assert args.transfer_threshold == (float(extra[extra.index("--transfer_threshold") + 1]) if "--transfer_threshold" in extra else 1.0)


@pytest.mark.parametrize("argv,named", [
    (["--dataset", "retrieval", "--transfer_masks"], "--transfer_masks"),                              # no mask path at all
    (["--dataset", "retrieval", "--transfer_masks"], "--query_mask_path"),                             # ... and where to put one
    (["--dataset", "retrieval", "--mask_path", "m", "--transfer_masks"], "--transfer_masks"),          # the triplet runs' mask path
    (["--dataset", "retrieval", "--mask_path", "m", "--transfer_masks"], "--query_mask_path"),
    (["--dataset", "cute", "--transfer_masks"], "--mask_path"),                                        # cute / nights still need --mask_path
    (["--dataset", "nights", "--query_mask_path", "q", "--transfer_masks"], "--mask_path"),
    (GOOD + ["--gallery_mask_path", "g"], "--transfer_masks"),
    (GOOD + ["--save_region_maps"], "--transfer_masks"),
    (GOOD + ["--save_region_matches"], "--transfer_masks"),
    (GOOD + ["--text_attn"], "--transfer_masks"),
    (GOOD + ["--taps", "up_blocks:0"], "--transfer_masks"),
    (GOOD + ["--metric", "clip_cross"], "--transfer_masks"),
    (GOOD + ["--metric", "dino_cross"], "--transfer_masks"),
    (GOOD + ["--metric", "diffeats", "--similarity", "cosine"], "--transfer_masks"),
    (GOOD + ["--metric", "dinofeats", "--similarity", "cosine"], "--transfer_masks"),
    (GOOD + ["--transfer_threshold", "nan"], "--transfer_threshold"),
    (["--dataset", "retrieval", "--query_mask_path", "q", "--save_transfer"], "--save_transfer"),      # needs --transfer_masks
    (["--dataset", "retrieval", "--query_mask_path", "q", "--save_transfer"], "--transfer_masks"),
    (["--dataset", "cute", "--mask_path", "m", "--transfer_masks", "--save_transfer"], "--save_transfer"),      # needs --dataset retrieval
])
def test_each_misuse_is_refused_with_code_2_and_the_flag_named(argv, named, capsys):
    from diffsim_amd.cli import arg_parse
    with pytest.raises(SystemExit) as e:
        arg_parse(argv)
    assert e.value.code == 2
    assert named in capsys.readouterr().err


def test_arguments_without_the_new_flags_parse_as_before():
    """--save_transfer is off as a class attribute of the parsed namespace and no entry of it, as --transfer_masks is: vars() of a run
    without the flags is what it was"""
    from diffsim_amd.cli import arg_parse
    for argv in ([], ["--dataset", "retrieval", "--query_mask_path", "q"], ["--dataset", "cute", "--mask_path", "m", "--transfer_masks"]):
        args = arg_parse(argv)
        assert "save_transfer" not in vars(args) and args.save_transfer is False, argv
    assert "save_transfer" in vars(arg_parse(GOOD + ["--save_transfer"]))
    assert sorted(set(vars(arg_parse(GOOD))) - set(vars(arg_parse(GOOD[:-1])))) == ["transfer_masks"]


# ---- the matrix's refusals come before any engine call
class _NoEngine:
    """a scorer whose every use is an error: the refusals below must not get that far"""
    exemplar_regions = True

    def __getattr__(self, name):
        raise AssertionError(f"the scorer was used ({name}) before the call was refused")


def test_an_exemplar_matrix_with_gallery_masks_is_refused_first():
    """score_path_matrix(exemplar=, masks_b=) is refused before anything is read; the latent form takes no gallery masks at all, and
    score_latent_matrix keeps the signature it had"""
    import inspect
    from diffsim_amd._lib import DsimError
    from diffsim_amd.retrieval import score_latent_matrix, score_latent_matrix_exemplar, score_path_matrix
    from diffsim_amd.transfer import ExemplarGuide
    lat = torch.zeros(2, 4, 8, 8)
    with pytest.raises(DsimError, match="masks_b"):
        score_path_matrix(_NoEngine(), ["a.png"], ["b.png"], 64, "p", masks_b=[None], exemplar=ExemplarGuide())
    with pytest.raises(DsimError, match="exemplar"):
        score_path_matrix(_NoEngine(), ["a.png"], ["b.png"], 64, "p", return_regions=True)
    with pytest.raises(TypeError, match="masks_b"):
        score_latent_matrix_exemplar(_NoEngine(), lat, lat, lat[:1], lat[:1], "p", masks_a=[None, None], masks_b=[None, None])
    a, x = inspect.signature(score_latent_matrix).parameters, inspect.signature(score_latent_matrix_exemplar).parameters
    assert "exemplar" not in a and list(x)[:12] == list(a)[:12]
    assert [n for n, q in x.items() if q.kind is q.KEYWORD_ONLY] == ["masks_a", "exemplar", "return_regions"]


def test_the_vit_and_feature_scorers_are_refused_first():
    from diffsim_amd.feats import FeatureView
    from diffsim_amd.retrieval import score_latent_matrix_exemplar, score_path_matrix
    from diffsim_amd.transfer import ExemplarGuide
    from diffsim_amd.vit import CLIPScore, Dinov2Score
    view = object.__new__(FeatureView)
    view.metric = "diffeats"
    lat = torch.zeros(2, 4, 8, 8)
    for scorer in (object.__new__(CLIPScore), object.__new__(Dinov2Score), view):
        with pytest.raises(NotImplementedError, match="regions"):
            score_latent_matrix_exemplar(scorer, lat, lat, lat[:1], lat[:1], "p", masks_a=[None, None], exemplar=ExemplarGuide())
        with pytest.raises(NotImplementedError, match="regions"):
            score_path_matrix(scorer, ["a.png"], ["b.png"], 64, "p", exemplar=ExemplarGuide())


# ---- the region rule on a matrix's masses
@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("thr", [0.0, 0.5, 1.0, 2.5])
def test_the_rule_on_cell_masses_is_the_rule_per_row(soft, thr):
    """(n_a n_b, N) masses with an exemplar's `full` repeated along its row against region_of_mass row by row: rows of a full
    exemplar, a non-finite row, a row where no token passes and ordinary rows"""
    from diffsim_amd.transfer import region_of_mass
    n_a, n_b, N = 3, 4, 49
    g = torch.Generator().manual_seed(5)
    mass = torch.rand(n_a, n_b, N, generator=g)
    mass[0, 1, 7] = float("nan")
    mass[2, 0] = 0.0                                              # no token passes a positive threshold of a zero mean ... or every one
    mass[2, 3] = 0.25                                             # every token at the mean
    full = torch.tensor([False, True, False])
    got = region_of_mass(mass.reshape(n_a * n_b, N), full.repeat_interleave(n_b), thr, soft).reshape(n_a, n_b, N)
    assert got.dtype == (torch.uint8 if soft else torch.bool)
    for i in range(n_a):
        for j in range(n_b):
            want = region_of_mass(mass[i, j][None], full[i:i + 1], thr, soft)[0]
            assert torch.equal(got[i, j], want), (i, j)
    whole = 255 if soft else True
    assert bool((got[1] == whole).all()) and bool((got[0, 1] == whole).all())
    if thr == 1.0:                                                # (uniform masses: about half of an ordinary row passes its mean)
        assert not bool((got[0, 0] == whole).all())
    if thr == 2.5:                                                # (none reaches 2.5 means: no token passes, the whole image)
        assert bool((got[0, 0] == whole).all())


def test_the_guide_accounts_alike_for_pairs_and_cells():
    from diffsim_amd.transfer import ExemplarGuide
    hard, soft = ExemplarGuide(), ExemplarGuide(soft=True)
    assert hard.on_fraction != hard.on_fraction                  # (NaN before any region)
    hard.account(torch.tensor([[True, False, False, False]]))
    hard.account(torch.ones(2, 3, 4, dtype=torch.bool))          # a matrix chunk's (n_a, n_b, N)
    assert hard.on_fraction == (1 + 24) / (4 + 24)
    soft.account(torch.tensor([[255, 0, 51, 0]], dtype=torch.uint8))
    assert abs(soft.on_fraction - (1 + 0.2) / 4) < 1e-12
    with pytest.raises(ValueError, match="rows"):
        hard.cell_regions(None, None, 2, torch.zeros(2, 9, dtype=torch.uint8))          # a hard guide takes bool rows


# ---- the binding
NEW = ["dsim_region_transfer_matrix", "dsim_score_matrix_cell_regions", "dsim_score_matrix_cell_weights"]


def _header_arity(name):
    text = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\(([^;]*?)\);", text, re.S)
    assert m, name
    params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return len([p for p in params.split(",") if p.strip()])


@pytest.mark.parametrize("name", NEW + [n + "_workspace_bytes" for n in NEW])
def test_lib_declares_the_new_symbols_with_the_headers_arity(name):
    from diffsim_amd import _lib
    table = next(v for v in vars(_lib).values() if isinstance(v, dict) and "dsim_score_matrix_regions" in v)
    assert name in table
    restype, argtypes = table[name]
    assert len(argtypes) == _header_arity(name), name
    assert restype is (_lib.C.c_size_t if name.endswith("_workspace_bytes") else _lib.C.c_int)


def test_the_abi_version_is_unchanged():
    text = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    assert re.search(r"#define DSIM_ABI_VERSION 7\b", text)
