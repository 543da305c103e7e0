"""Exemplar-guided regions, host side (no GPU): the C ABI's two entry points and their refusals, the command line's two flags, the
region rule on hand-made masses, the scorers that must refuse, and tests/_transfer64.py itself -- its masses against a hand-written
softmax, a plain float32 restatement of the kernels' arithmetic inside its bound on every shape of the GPU tests, and the planted
family's premise on the reference alone."""
import ctypes
import os
import re

import pytest
import torch

from tests import _align64 as A
from tests import _transfer64 as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(N, H, D, dt) for (N, H, D), dts in A.SHAPES.items() for dt in dts]


def test_header_declares_and_lib_binds_the_transfer_entry_points():
    hdr = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    assert re.search(r"size_t\s+dsim_pair_region_transfer_workspace_bytes\s*\(\s*int n_feat,\s*int n_pairs,\s*int B,\s*int H,\s*int N,"
                     r"\s*int D\)", hdr)
    decl = re.search(r"int\s+dsim_pair_region_transfer\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl).split(",")) == 18
    assert re.search(r"#define\s+DSIM_ABI_VERSION\s+7\b", hdr)             # additive: the version stays
    from diffsim_amd import _lib
    assert _lib.ABI_VERSION == 7
    assert len(_lib.SYMBOLS["dsim_pair_region_transfer_workspace_bytes"][1]) == 6
    assert len(_lib.SYMBOLS["dsim_pair_region_transfer"][1]) == 18
    L = _lib.lib()
    assert L.dsim_pair_region_transfer and L.dsim_pair_region_transfer_workspace_bytes


def test_refusals_come_before_any_launch():
    """Every refusal is decided on the host before anything is enqueued, so it can be checked without a GPU (the pointers are never
    read): the workspace query's zeros, a short workspace, the shape and dtype refusals of dsim_pair_align, directions outside 1 .. 3,
    a NULL weights or mass."""
    from diffsim_amd import _lib
    L = _lib.lib()
    B, H, N, D = 2, 4, 64, 32
    assert L.dsim_pair_region_transfer_workspace_bytes(2, 1, B, H, N, D) >= 2 * B * H * N * 4
    for shape in ((2, 0, B, H, N, D), (2, 1, B, H, N, 24), (2, 1, B, H, 0, D), (0, 1, B, H, N, D), (2, 40000, B, H, N, D),
                  (1 << 20, 1, B, H, 1 << 11, D)):
        assert L.dsim_pair_region_transfer_workspace_bytes(*shape) == 0, shape
    need = int(L.dsim_pair_region_transfer_workspace_bytes(2, 1, B, H, N, D))
    fake = ctypes.c_void_p(0x10000)

    def go(n=1, n_feat=2, N=N, D=D, dirs=3, w=fake, mass=fake, ws=need, dtype=_lib.DSIM_BF16):
        rc = L.dsim_pair_region_transfer(fake, fake, w, n_feat, fake, fake, n, B, H, N, D, dtype, dirs, mass, None, fake, ws, None)
        return L.dsim_strerror(rc).lower()

    assert b"workspace" in go(ws=need // 2)
    for kw in (dict(D=24), dict(dtype=7), dict(n=0), dict(n=40000), dict(n_feat=0), dict(dirs=0), dict(dirs=4), dict(dirs=-1),
               dict(w=None), dict(mass=None)):
        for dtype in ((kw["dtype"],) if "dtype" in kw else (_lib.DSIM_BF16, _lib.DSIM_F16, _lib.DSIM_F32)):
            assert b"invalid" in go(**{**kw, "dtype": dtype}), (kw, dtype)


# ---- the command line
GOOD = ["--dataset", "cute", "--mask_path", "m", "--transfer_masks"]


def test_arguments_without_the_flags_parse_as_before():
    from diffsim_amd.cli import arg_parse
    ns = vars(arg_parse([]))
    assert "transfer_masks" not in ns and "transfer_threshold" not in ns
    args = arg_parse([])
    assert args.transfer_masks is False and args.transfer_threshold == 1.0          # (the off values: class attributes of _Args)


@pytest.mark.parametrize("extra", [[], ["--transfer_threshold", "0.5"], ["--soft_masks"], ["--dataset", "nights"],
                                   ["--metric", "diffsim_xl"], ["--metric", "dit"], ["--transfer_threshold", "0"]])
def test_the_flags_are_accepted_with_their_partners(extra):
    from diffsim_amd.cli import arg_parse
    args = arg_parse(GOOD + extra)
    assert args.transfer_masks is True and args.use_mask is True
    assert args.transfer_threshold == (float(extra[1]) if extra[:1] == ["--transfer_threshold"] else 1.0)


@pytest.mark.parametrize("argv,named", [
    (["--dataset", "cute", "--transfer_masks"], "--transfer_masks"),                                # no --mask_path
    (["--dataset", "cute", "--mask_path", "m", "--transfer_threshold", "2"], "--transfer_threshold"),      # the threshold alone
    (["--mask_path", "m", "--transfer_masks", "--dataset", "sref"], "--transfer_masks"),
    (["--mask_path", "m", "--transfer_masks", "--dataset", "retrieval"], "--transfer_masks"),
    (GOOD + ["--taps", "up_blocks:0"], "--transfer_masks"),
    (GOOD + ["--text_attn"], "--transfer_masks"),
    (GOOD + ["--metric", "clip_cross"], "--transfer_masks"),
    (GOOD + ["--metric", "dino_cross"], "--transfer_masks"),
    (GOOD + ["--metric", "diffeats", "--similarity", "cosine"], "--transfer_masks"),
    (GOOD + ["--metric", "dinofeats", "--similarity", "cosine"], "--transfer_masks"),
    (GOOD + ["--transfer_threshold", "nan"], "--transfer_threshold"),
    (GOOD + ["--transfer_threshold", "inf"], "--transfer_threshold"),
    (GOOD + ["--transfer_threshold", "-0.5"], "--transfer_threshold"),
])
def test_each_misuse_is_refused_with_code_2_and_the_flag_named(argv, named, capsys):
    from diffsim_amd.cli import arg_parse
    with pytest.raises(SystemExit) as e:
        arg_parse(argv)
    assert e.value.code == 2
    assert named in capsys.readouterr().err


# ---- the scorers that must refuse, the guide's own checks
def test_the_vit_and_feature_metrics_have_no_exemplar_regions():
    from diffsim_amd import transfer
    from diffsim_amd.feats import FeatureView
    from diffsim_amd.vit import CLIPScore, Dinov2Score
    view = object.__new__(FeatureView)
    view.metric = "diffeats"
    for scorer in (object.__new__(CLIPScore), object.__new__(Dinov2Score), view):
        for call in (scorer.exemplar_region_score, scorer.transferred_region):
            with pytest.raises(NotImplementedError, match="regions"):
                call("a.png", "b.png", None, 64, "p", "up_blocks", 0, 100)
        with pytest.raises(NotImplementedError, match="regions"):
            transfer.require_exemplar_regions(scorer)
        with pytest.raises(NotImplementedError, match="regions"):
            transfer.score_path_pairs_exemplar(scorer, [("a.png", "b.png")], None, 64, "p")
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.diffsim_dit import diffsim_DiT
    from diffsim_amd.diffsim_xl import diffsim_xl
    for kind in (DiffSim, diffsim_xl, diffsim_DiT):
        transfer.require_exemplar_regions(object.__new__(kind))
        assert callable(kind.exemplar_region_score) and callable(kind.transferred_region)


def test_the_guide_validates_its_threshold_as_textguide_does():
    from diffsim_amd.transfer import ExemplarGuide
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rel_threshold"):
            ExemplarGuide(bad)
    g = ExemplarGuide()
    assert g.rel_threshold == 1.0 and g.soft is False and g.on_fraction != g.on_fraction
    with pytest.raises(ValueError):
        g.regions(None, None, 1, torch.zeros(2, 4, dtype=torch.uint8), torch.tensor([0], dtype=torch.int32), torch.tensor([1], dtype=torch.int32))


def test_the_harness_refuses_an_exemplar_with_text_or_mask_triples():
    from diffsim_amd import harness as H
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.transfer import ExemplarGuide
    scorer, trip = object.__new__(DiffSim), [("a", "b", "c", "p")]
    for kw, msg in ((dict(masks=[None], text=object()), "text"), (dict(masks=[("a", "b", "c")]), "triples"), (dict(), "masks"),
                    (dict(masks=[None], soft=True), "soft")):
        with pytest.raises(ValueError, match=msg):
            H.score_path_triplets(scorer, trip, 64, "up_blocks", 0, 100, exemplar=ExemplarGuide(), **kw)


# ---- the region rule on hand-made masses
def test_the_region_rule():
    from diffsim_amd.transfer import region_of_mass
    """threshold 0, a tie at the mean, nothing passing, a NaN, a full exemplar; the soft bytes of the same cases."""
    no = torch.zeros(1, dtype=torch.bool)
    # a tie at the mean: values whose float64 mean is exactly one of them
    t = torch.tensor([[0.25, 0.5, 0.75, 0.5]])
    assert region_of_mass(t, no, 1.0).tolist() == [[False, True, True, True]]
    assert region_of_mass(t, no, 0.0).tolist() == [[True] * 4]                        # threshold 0: every token
    assert region_of_mass(t, no, 1.5).tolist() == [[False, False, True, False]]       # 0.75 >= 1.5 x 0.5, a tie again
    assert region_of_mass(t, no, 1.6).tolist() == [[True] * 4]                        # nothing passes: the whole image
    assert region_of_mass(torch.tensor([[0.25, float("nan"), 0.75, 0.5]]), no, 1.0).tolist() == [[True] * 4]
    assert region_of_mass(torch.tensor([[0.25, float("inf"), 0.75, 0.5]]), no, 1.0).tolist() == [[True] * 4]
    assert region_of_mass(t, ~no, 1.0).tolist() == [[True] * 4]                       # a full exemplar: whole, whatever the mass
    # soft: 255 where the hard rule says on, the share of the threshold elsewhere; whole rows all 255
    assert region_of_mass(t, no, 1.0, soft=True).tolist() == [[128, 255, 255, 255]]
    assert region_of_mass(t, no, 1.6, soft=True).tolist() == [[255] * 4]
    assert region_of_mass(t, ~no, 1.0, soft=True).tolist() == [[255] * 4]


def test_the_first_case_of_the_region_rule_is_decided_in_float64():
    """0.3f is 0.300000011920929; the float64 mean of (0.1f, 0.2f, 0.3f, 0.6f) is 0.3000000081956387: the third token passes, by the
    f32 values as they are -- the rule is s >= threshold x mean on the stored values, nothing else."""
    from diffsim_amd.transfer import region_of_mass
    s = torch.tensor([[0.1, 0.2, 0.3, 0.6]])
    mean = s.double().mean().item()
    want = [[float(v) >= mean for v in s[0].double()]]
    assert region_of_mass(s, torch.zeros(1, dtype=torch.bool), 1.0).tolist() == want


def test_full_and_empty_exemplars_skip_the_kernel():
    """A fully-on exemplar makes the other image whole, and an empty exemplar is the whole image and then does the same: neither
    reaches the kernel, so the rows come out on the CPU, where a launch would raise."""
    from diffsim_amd.transfer import ExemplarGuide
    ia, ib = torch.tensor([0, 2], dtype=torch.int32), torch.tensor([1, 3], dtype=torch.int32)
    rows = torch.tensor([[1, 1, 1, 1], [0, 1, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0]], dtype=torch.bool)
    g = ExemplarGuide()
    out, mass = g.regions(None, None, 2, rows, ia, ib, return_mass=True)
    assert out.dtype == torch.bool and out.tolist() == [[True] * 4] * 4
    assert mass.tolist() == [[1.0] * 4] * 2 and g.on_fraction == 1.0
    soft = torch.tensor([[255] * 4, [0, 9, 0, 0], [0] * 4, [7, 0, 0, 0]], dtype=torch.uint8)
    gs = ExemplarGuide(soft=True)
    assert gs.regions(None, None, 2, soft, ia, ib).tolist() == [[255] * 4] * 4 and gs.on_fraction == 1.0
    with pytest.raises(Exception):                                           # a partial exemplar needs the kernel
        ExemplarGuide().regions(torch.zeros(4, 2, 4, 32), torch.zeros(4, 2, 4, 32), 2, rows.flip(0), ia, ib)


# ---- tests/_transfer64.py itself
def test_mass64_against_a_hand_written_two_head_softmax():
    """3 tokens, 2 heads of dim 1, B = 1: every probability written out."""
    import math
    q = torch.tensor([[[[1.0, 2.0], [0.0, -1.0], [2.0, 0.5]]], [[[0.5, 1.0], [1.0, 1.0], [-1.0, 2.0]]]])      # [2][1][3][2]
    k = torch.tensor([[[[1.0, 0.0], [2.0, 1.0], [-1.0, 3.0]]], [[[0.0, 1.0], [1.0, -2.0], [3.0, 0.5]]]])
    w = torch.tensor([[255, 0, 51], [0, 255, 102]], dtype=torch.uint8)
    mass, _ = T.mass64(q, k, w, [(0, 1)], 2, with_bound=False)

    def hand(qi, kx, wx):
        out = []
        for i in range(3):
            r = 0.0
            for h in range(2):
                e = [math.exp(float(qi[0, i, h]) * float(kx[0, j, h])) for j in range(3)]         # D = 1: scale 1
                r += sum(e[j] * float(wx[j]) / 255.0 for j in range(3)) / sum(e)
            out.append(r / 2)
        return out
    assert torch.allclose(mass[0, 0], torch.tensor(hand(q[0], k[1], w[1]), dtype=torch.float64), rtol=1e-14, atol=0)
    assert torch.allclose(mass[0, 1], torch.tensor(hand(q[1], k[0], w[0]), dtype=torch.float64), rtol=1e-14, atol=0)
    full, _ = T.mass64(q, k, torch.full_like(w, 255), [(0, 1)], 2, with_bound=False)
    assert (full - 1).abs().max() < 1e-15


@pytest.mark.parametrize("N,H,D,dtype", CASES, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("scale", [1.0, 14.0])
def test_a_float32_restatement_stays_inside_the_bound(N, H, D, dtype, scale):
    """The kernels' arithmetic in plain float32 torch against float64, one pair, both directions, random bytes: the bound suffices for
    f32 arithmetic without the kernel."""
    q, k = A.feats(2, 11, dtype, N, H, D, scale)
    w = T.random_bytes(2, N, 5)
    ref, bound = T.mass64(q, k, w, [(0, 1)], H)
    got = torch.stack([T.direction_mass32(q[0], k[1], w[1], H), T.direction_mass32(q[1], k[0], w[0], H)]).double()
    ratio = ((got - ref[0]).abs() / bound[0]).max().item()
    print(f"N={N} H={H} D={D} {dtype} scale={scale}: largest |f32 - f64| / bound = {ratio:.4f}")
    assert ratio <= 1.0
    assert 0 <= ref.min() and ref.max() <= 1 + 1e-12 and bound.max() < 1e-3


@pytest.mark.parametrize("N,H,D", list(A.PLANTED), ids=str)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=lambda v: str(v).replace("torch.", ""))
def test_planted_margins(N, H, D, dtype):
    """The premise of the planted GPU test, on the reference alone: with exactly N // 2 exemplar tokens on, every on-token's image
    has mass >= 0.75 and every other token <= 0.25 (a top weight of 0.75 on every row: 0.25 + 0.75 f <= 0.75 and 0.75 f > 0.25 for
    f = 1/2), and the hard rule at threshold 1.0 separates them with a margin above the bound."""
    q, k, pi = A.planted(3, dtype, N, H, D, A.PLANTED[(N, H, D)])
    g = torch.Generator().manual_seed(17)
    m0 = torch.zeros(N, dtype=torch.bool)
    m0[torch.randperm(N, generator=g)[:N // 2]] = True
    w = torch.stack([m0, torch.ones(N, dtype=torch.bool)]).to(torch.uint8) * 255
    mass, bound = T.mass64(q, k, w, [(0, 1)], H)
    s, b = mass[0, 1], bound[0, 1]                                     # on image 1's grid
    want = torch.zeros(N, dtype=torch.bool)
    want[pi] = m0
    assert s[want].min() >= 0.75 and s[~want].max() <= 0.25
    mean = s.mean()
    margin = torch.minimum(s[want].min() - mean, mean - s[~want].max())
    assert margin > 0.1 and margin > 100 * (b.max() + b.mean())        # (the mean moves by at most the mean bound)
    from diffsim_amd.transfer import region_of_mass
    assert torch.equal(region_of_mass(s.float()[None], torch.zeros(1, dtype=torch.bool), 1.0)[0], want)
