"""Region score matrices, host side (no GPU): the C ABI's two entry points and their refusals, the command line's
--query_mask_path / --gallery_mask_path, the mask lookup under separate query and gallery roots, engine.score_matrix_regions'
own checks, retrieval's masks_a / masks_b on a CPU stand-in, and tests/_region64.py's cells with full masks against
tests/_tail64.py (the yardstick of tests/test_gpu_region_matrix.py, checked here)."""
import os
import re

import pytest
import torch

from tests._region64 import Region64
from tests._tail64 import Tail64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_lib_binds_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    assert re.search(r"size_t\s+dsim_score_matrix_regions_workspace_bytes\s*\(\s*int n_a,\s*int n_b,\s*int B,\s*int H,\s*int N,\s*int D,"
                     r"\s*int dtype\)", hdr)
    assert re.search(r"#define\s+DSIM_ABI_VERSION\s+7\b", hdr)             # additive: the version stays
    from diffsim_amd import _lib
    assert len(_lib.SYMBOLS["dsim_score_matrix_regions_workspace_bytes"][1]) == 7
    assert len(_lib.SYMBOLS["dsim_score_matrix_regions"][1]) == 22
    decl = re.search(r"int\s+dsim_score_matrix_regions\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 22


def test_refusals_come_before_any_launch():
    """Every refusal of dsim_score_matrix_regions is decided on the host before anything is enqueued, so it is checked without a GPU
    (the pointers are never read)."""
    import ctypes
    from diffsim_amd import _lib
    L = _lib.lib()
    B, H, N, D = 2, 4, 64, 32
    bf16 = _lib.DSIM_BF16
    wsb = L.dsim_score_matrix_regions_workspace_bytes
    need = int(wsb(3, 2, B, H, N, D, bf16))
    # lists, counts, the two cell-index arrays, the self outputs of both sets, the partials, the slack
    parts = (5 * N * 4, 5 * 4, 6 * 4, 6 * 4, 3 * B * N * H * D * 2, 2 * B * N * H * D * 2, 6 * 2 * B * H * 4 * 4)
    assert need == sum((p + 255) // 256 * 256 for p in parts) + 256
    assert int(wsb(3, 2, B, H, N, D, _lib.DSIM_F32)) > need                  # (f32 self outputs)
    assert int(wsb(3, 2, B, H, N, D, _lib.DSIM_F16)) == need
    big = 32767
    for args in ((0, 2, B, H, N, D, bf16), (3, 0, B, H, N, D, bf16), (3, 2, B, H, N, 24, bf16), (3, 2, B, H, N, 0, bf16),
                 (3, 2, B, H, 0, D, bf16), (3, 2, 0, H, N, D, bf16), (3, 2, B, H, N, D, 9), (3, 2, B, H, N, D, -1),
                 (65535, 1, 1, 1, 1, 16, bf16),                              # n_a + n_b > 65535
                 (3, 2, 2, 32768, N, 16, bf16),                              # B H > 65535
                 (big, big, 1, 1, 256, 16, bf16),                            # the cross grid: ~2^30 cells x 2 directions x 2 query tiles
                 (3, 2, 1, 1, 1 << 27, 16, bf16)):                           # a set's features: 3 x 2^27 x 16 elements >= 2^31
        assert wsb(*args) == 0, args
    assert wsb(65534, 1, 1, 1, 1, 16, bf16) > 0 and wsb(3, 2, 1, 65535, N, 16, bf16) > 0
    fake = ctypes.c_void_p(0x10000)

    def go(n_a=3, n_b=2, H=H, N=N, D=D, dtype=bf16, sim=0, ws=need, mask_a=fake, out=fake):
        rc = L.dsim_score_matrix_regions(fake, fake, fake, mask_a, n_a, fake, fake, fake, fake, n_b, B, H, N, D, dtype, sim, out, None,
                                         None, fake, ws, None)
        return L.dsim_strerror(rc).lower()

    assert b"workspace" in go(ws=need // 2)
    assert b"workspace" in go(ws=need - 257)          # (the query adds 256 bytes of alignment slack; the pointer here is aligned)
    for kw in (dict(dtype=9), dict(dtype=-1), dict(sim=2), dict(sim=-1), dict(D=24), dict(D=0), dict(n_a=0), dict(n_b=0), dict(n_a=-3),
               dict(n_a=65535, ws=1 << 44), dict(H=32768, ws=1 << 44), dict(n_a=big, n_b=big, N=256, ws=1 << 50), dict(mask_a=None),
               dict(out=None)):
        for dtype in ((bf16, _lib.DSIM_F16, _lib.DSIM_F32) if "dtype" not in kw else (kw["dtype"],)):
            assert b"invalid" in go(**{**kw, "dtype": dtype}), (kw, dtype)


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_the_two_mask_flags_are_for_retrieval(capsys):
    from diffsim_amd.cli import arg_parse
    base = ["--dataset", "retrieval", "--image_path", "g", "--query_path", "q", "--out_path", "o"]
    a = arg_parse(base + ["--query_mask_path", "qm"])
    assert (a.query_mask_path, a.gallery_mask_path) == ("qm", None)
    a = arg_parse(base + ["--gallery_mask_path", "gm"])
    assert (a.query_mask_path, a.gallery_mask_path) == (None, "gm")
    a = arg_parse(base + ["--query_mask_path", "qm", "--gallery_mask_path", "gm"])
    assert (a.query_mask_path, a.gallery_mask_path) == ("qm", "gm") and a.mask_path is None
    a = arg_parse(base)
    assert (a.query_mask_path, a.gallery_mask_path) == (None, None)

    def refused(argv, named):
        with pytest.raises(SystemExit) as e:
            arg_parse(argv)
        assert e.value.code == 2
        msg = capsys.readouterr().err.split("error:")[-1]                    # (the message, not the usage text above it)
        assert named in msg, (argv, msg)

    for flag in ("--query_mask_path", "--gallery_mask_path"):
        for dataset in ("cute", "nights", "sref"):
            refused(["--dataset", dataset, flag, "m"], flag)
        refused([flag, "m"], flag)                                           # (the default dataset)
        for extra in (["--save_maps"], ["--save_matches"], ["--text_attn"], ["--text_attn", "cat"]):
            refused(base + [flag, "m"] + extra, flag)
    refused(["--dataset", "retrieval", "--mask_path", "m"], "--mask_path")
    refused(base + ["--mask_path", "m", "--query_mask_path", "qm"], "--mask_path")
    with pytest.raises(SystemExit):
        arg_parse(["--dataset", "retrieval", "--mask_path", "m"])
    assert "--query_mask_path" in capsys.readouterr().err.split("error:")[-1]                  # ... and points at the new flags


def test_mask_lookup_under_separate_query_and_gallery_roots(tmp_path):
    from diffsim_amd.regions import mask_path_for
    q, g, qm, gm = (tmp_path / d for d in ("q", "g", "qm", "gm"))
    for root, rels in ((q, ("a/x.jpg", "y.png")), (g, ("a/x.jpg", "b/z.jpeg")), (qm, ("a/x.png", "y.png")), (gm, ("a/x.jpg",))):
        for rel in rels:
            (root / rel).parent.mkdir(parents=True, exist_ok=True)
            (root / rel).write_bytes(b"")
    assert mask_path_for(str(q / "a/x.jpg"), str(q), str(qm)) == str(qm / "a/x.png")
    assert mask_path_for(str(q / "y.png"), str(q), str(qm)) == str(qm / "y.png")
    assert mask_path_for(str(g / "a/x.jpg"), str(g), str(gm)) == str(gm / "a/x.jpg")         # the same relative name, the gallery's folder
    assert mask_path_for(str(g / "b/z.jpeg"), str(g), str(gm)) is None                       # a missing file: the whole image
    assert mask_path_for(str(q / "y.png"), str(q), str(gm)) is None


# ---- engine.score_matrix_regions' own checks ------------------------------------------------------------------------------------------
def test_engine_checks_come_before_the_library(monkeypatch):
    from diffsim_amd import _lib, engine
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was touched"))
    N, H, D = 16, 2, 8
    fa = tuple(torch.zeros(2, 2, N, H * D) for _ in range(3))
    fb = tuple(torch.zeros(3, 2, N, H * D) for _ in range(3))
    ma, mb = torch.ones(2, N, dtype=torch.bool), torch.ones(3, N, dtype=torch.uint8)
    with pytest.raises(_lib.DsimError, match="not on the GPU"):
        engine.score_matrix_regions(fa, fb, ma, mb, H)
    with pytest.raises(_lib.DsimError, match=r"mask_b must be \(n, N\) = \(3, 16\)"):
        engine.score_matrix_regions(fa, fb, ma, mb[:2], H)
    with pytest.raises(_lib.DsimError, match=r"mask_a must be \(n, N\)"):
        engine.score_matrix_regions(fa, fb, ma[:, :8], mb, H)
    with pytest.raises(_lib.DsimError, match=r"mask_a must be \(n, N\)"):
        engine.score_matrix_regions(fa, fb, ma.view(2, 4, 4), mb, H)
    with pytest.raises(_lib.DsimError, match="mask_a must be bool or uint8"):
        engine.score_matrix_regions(fa, fb, ma.float(), mb, H)
    with pytest.raises(_lib.DsimError, match="mask_b must be bool or uint8"):
        engine.score_matrix_regions(fa, fb, ma, mb.int(), H)
    with pytest.raises(_lib.DsimError, match="one geometry"):
        engine.score_matrix_regions(fa, tuple(t[:, :, :8] for t in fb), ma, mb, H)
    with pytest.raises(ValueError):
        engine.score_matrix_regions(fa, fb, ma, mb, H, "l1")


# ---- retrieval's masks on a CPU stand-in ------------------------------------------------------------------------------------------------
class _Scorer:
    """what score_latent_matrix asks of a scorer: features that are the latents' own rows, on the CPU"""
    device = torch.device("cpu")
    H, D, side = 2, 8, 4

    def tap_of(self, block, layer):
        return (block, layer)

    def bind_prompt(self, prompt, n, what):
        return prompt

    def engine_at(self, tap):
        return type("E", (), {"heads": self.H})()

    def sweep_engine(self, taps, side):
        return None, [(self.side * self.side, self.H, self.D)]

    def auto_rows(self, eng, n, k):
        return 1

    def tap_features(self, lat, noise, prompt, tap, step):
        n = lat.shape[0]
        g = torch.Generator().manual_seed(0)
        w = torch.randn(3, lat[0].numel(), 2 * self.side * self.side * self.H * self.D, generator=g)
        x = (lat + noise).reshape(n, 1, -1)                  # (one product per image: its bits do not depend on the batch)
        return tuple(torch.cat([x[j] @ w[i] for j in range(n)]).view(n, 2, self.side * self.side, self.H * self.D) for i in range(3))


def test_latent_matrix_masks_reach_the_region_matrix_and_none_changes_nothing(monkeypatch):
    from diffsim_amd import retrieval as R
    calls = []

    def matrix(fa, fb, heads, sim, return_status=False):
        calls.append(("whole", fa[0].shape[0], fb[0].shape[0]))
        return torch.zeros(fa[0].shape[0], fb[0].shape[0]), torch.zeros(fa[0].shape[0], fb[0].shape[0], dtype=torch.int32)

    def regions(fa, fb, ma, mb, heads, sim, return_status=False):
        calls.append(("regions", ma.clone(), mb.clone()))
        r = Region64(*(torch.cat([a, b]) for a, b in zip(fa, fb)), torch.cat([ma, mb]), heads, torch.float32)
        n_a, n_b = ma.shape[0], mb.shape[0]
        s = torch.tensor([[r.pair(i, n_a + j, sim) for j in range(n_b)] for i in range(n_a)], dtype=torch.float32)
        return s, torch.zeros(n_a, n_b, dtype=torch.int32)

    monkeypatch.setattr(R, "score_matrix", matrix)
    monkeypatch.setattr(R, "score_matrix_regions", regions)
    monkeypatch.setattr(R, "score_matrix_workspace_bytes", lambda *a: 0)
    monkeypatch.setattr(R, "score_matrix_regions_workspace_bytes", lambda *a: 0)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev=None: (1 << 40, 1 << 40))
    sc = _Scorer()
    g = torch.Generator().manual_seed(3)
    la, lb, nz = torch.randn(2, 4, 4, 4, generator=g), torch.randn(3, 4, 4, 4, generator=g), torch.randn(1, 4, 4, 4, generator=g)
    m, bad = R.score_latent_matrix(sc, la, lb, nz, nz, "p", batch=2, return_status=True)
    assert [c[0] for c in calls] == ["whole", "whole"] and bad == 0          # two gallery chunks, the unmasked path
    calls.clear()
    mA = torch.rand(2, 4, 4, generator=g) < 0.5
    mA[0] = False                                                            # nothing on: the whole image
    mB = [None, (torch.rand(16, generator=g) < 0.5).numpy(), torch.ones(4, 4, dtype=torch.bool)]
    both = R.score_latent_matrix(sc, la, lb, nz, nz, "p", batch=2, masks_a=mA, masks_b=mB)
    assert [c[0] for c in calls] == ["regions", "regions"]
    assert calls[0][1].all(1).tolist() == [True, False] and torch.equal(calls[0][1][1], mA[1].flatten())
    assert calls[0][2].shape == (2, 16) and calls[1][2].shape == (1, 16)     # the gallery's masks sliced as its latents are
    assert torch.equal(calls[0][2][1], torch.as_tensor(mB[1])) and calls[1][2].all() and calls[0][2][0].all()
    one = R.score_latent_matrix(sc, la, lb, nz, nz, "p", batch=3, masks_a=mA, masks_b=mB)
    assert torch.equal(one, both)
    calls.clear()
    only_b = R.score_latent_matrix(sc, la, lb, nz, nz, "p", masks_b=mB)
    assert calls[0][0] == "regions" and calls[0][1].all()                    # the other side: whole images
    assert not torch.equal(only_b, both)
    with pytest.raises(ValueError, match="masks_a"):
        R.score_latent_matrix(sc, la, lb, nz, nz, "p", masks_a=mA[:1])
    with pytest.raises(ValueError, match="token grid"):
        R.score_latent_matrix(sc, la, lb, nz, nz, "p", masks_b=[None, torch.ones(3, 3), None])
    with pytest.raises(TypeError):
        R.score_latent_matrix(sc, la, lb, nz, nz, "p", "up_blocks", 0, 600, "cosine", None, False, mA)      # keyword-only


# ---- the float64 yardstick itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("sim", ["cosine", "mse"])
def test_region64_cells_with_full_masks_are_tail64_pairs(dtype, sim):
    N, H, D = 49, 2, 16
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(5, 2, N, H * D, generator=g).to(dtype) for _ in range(3))
    full = torch.ones(5, N, dtype=torch.uint8) * 255
    t, r = Tail64(q, k, v, H, dtype), Region64(q, k, v, full, H, dtype)
    for i in range(2):                                      # set A: images 0, 1; set B: images 2, 3, 4
        for j in range(3):
            assert r.pair(i, 2 + j, sim) == t.pair(i, 2 + j, sim)[0]
