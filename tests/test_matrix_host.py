"""Score matrices, host side (no GPU): the C ABI's two entry points, their workspace layout and refusals (one shape check for the
queries, the launchers and the entry points), the ranking rules and files, the image walk and the --dataset retrieval command line."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_binds_the_matrix_entry_points():
    hdr = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    assert re.search(r"size_t\s+dsim_score_matrix_workspace_bytes\s*\(\s*int n_a,\s*int n_b,\s*int B,\s*int H,\s*int N,\s*int D,\s*int dtype\)", hdr)
    assert re.search(r"int\s+dsim_score_matrix\s*\(", hdr)
    assert re.search(r"#define\s+DSIM_ABI_VERSION\s+7\b", hdr)
    from diffsim_amd import _lib
    assert "dsim_score_matrix" in _lib.SYMBOLS and "dsim_score_matrix_workspace_bytes" in _lib.SYMBOLS
    assert len(_lib.SYMBOLS["dsim_score_matrix"][1]) == 19
    assert len(_lib.SYMBOLS["dsim_score_matrix_workspace_bytes"][1]) == 7


# ---- the workspace queries and the refusals: one layout, one shape check --------------------------------------------------------------
SHAPE = (3, 2, 2, 4, 64, 32)                   # (n_a, n_b, B, H, N, D): a tiled shape
BF16, F16, F32 = 1, 2, 0                       # include/diffsim_amd.h's dtype codes (checked below against _lib's)


def _up(b):
    return (b + 255) // 256 * 256


def _tiled_bytes(n_a, n_b, B, H, N, D, es):
    """self A | self B | partials [n_cells][2][B H][qtiles][4] f32, each 256-byte aligned, and the query's 256 bytes of slack"""
    image = B * N * H * D * es
    return _up(n_a * image) + _up(n_b * image) + _up(n_a * n_b * 2 * B * H * ((N + 127) // 128) * 4 * 4) + 256


def _listed_extra(n_a, n_b, N):
    """lists [n_a + n_b][N] | counts [n_a + n_b] | cell indices [2][n_cells], int32, each 256-byte aligned"""
    return _up((n_a + n_b) * N * 4) + _up((n_a + n_b) * 4) + 2 * _up(n_a * n_b * 4)


def _refused():
    """arguments (n_a, n_b, B, H, N, D, dtype) that no matrix call serves"""
    n_a, n_b, B, H, N, D = SHAPE
    big = 32767
    return ((0, n_b, B, H, N, D, BF16), (-3, n_b, B, H, N, D, BF16), (n_a, 0, B, H, N, D, BF16), (n_a, n_b, 0, H, N, D, BF16),
            (n_a, n_b, B, 0, N, D, BF16), (n_a, n_b, B, H, 0, D, BF16), (n_a, n_b, B, H, N, 0, BF16), (n_a, n_b, B, H, N, 24, BF16),
            (n_a, n_b, B, H, N, D, -1), (n_a, n_b, B, H, N, D, 9),
            (65535, 1, 1, 1, 1, 16, BF16),                              # n_a + n_b > 65535
            (n_a, n_b, 2, 32768, N, 16, BF16),                          # a tiled B H > 65535
            (big, big, 1, 1, 256, 16, BF16),                            # the cross grid: ~2^30 cells x 2 directions x 2 query tiles
            (8192, 8192, 1, 1, 2049, 16, BF16))                         # ... alone: 2^26 cells x 2 x 17 tiles, every other bound met


def test_workspace_query_is_the_layout():
    from diffsim_amd import _lib
    assert (_lib.DSIM_BF16, _lib.DSIM_F16, _lib.DSIM_F32) == (BF16, F16, F32)
    wsb = _lib.lib().dsim_score_matrix_workspace_bytes
    need = int(wsb(*SHAPE, BF16))
    assert need == _tiled_bytes(*SHAPE, 2)
    assert int(wsb(*SHAPE, F16)) == need
    assert int(wsb(*SHAPE, F32)) == _tiled_bytes(*SHAPE, 4) > need          # (f32 self outputs)


@pytest.mark.parametrize("shape", [SHAPE, (2, 3, 2, 2, 129, 16)])
def test_regions_query_adds_the_lists_counts_and_cell_indices(shape):
    from diffsim_amd import _lib
    L = _lib.lib()
    n_a, n_b, _, _, N, _ = shape
    for dtype in (BF16, F16, F32):
        plain = int(L.dsim_score_matrix_workspace_bytes(*shape, dtype))
        assert plain > 0
        assert int(L.dsim_score_matrix_regions_workspace_bytes(*shape, dtype)) - plain == _listed_extra(n_a, n_b, N)


def test_workspace_query_is_zero_exactly_where_the_call_is_refused():
    from diffsim_amd import _lib
    wsb = _lib.lib().dsim_score_matrix_workspace_bytes
    for args in _refused():
        assert wsb(*args) == 0, args
    assert wsb(65534, 1, 1, 1, 1, 16, BF16) > 0 and wsb(3, 2, 1, 65535, 64, 16, BF16) > 0      # just inside the two grid bounds
    assert wsb(8192, 8192, 1, 1, 1920, 16, BF16) > 0                                            # ... and the cross grid's: 15 tiles


@pytest.mark.parametrize("dtype", [BF16, F16, F32])
def test_matrix_refusals_come_before_any_launch(dtype):
    """Every refusal of dsim_score_matrix is decided on the host before anything is enqueued, so it is checked without a GPU (the
    pointers are never read)."""
    import ctypes
    from diffsim_amd import _lib
    L = _lib.lib()
    need = int(L.dsim_score_matrix_workspace_bytes(*SHAPE, dtype))
    fake = ctypes.c_void_p(0x10000)

    def go(shape=SHAPE, dtype=dtype, sim=0, ws=need, qa=fake, out=fake):
        n_a, n_b, B, H, N, D = shape
        rc = L.dsim_score_matrix(qa, fake, fake, n_a, fake, fake, fake, n_b, B, H, N, D, dtype, sim, out, None, fake, ws, None)
        return L.dsim_strerror(rc).lower()

    assert b"workspace" in go(ws=need // 2)
    assert b"workspace" in go(ws=need - 257)          # (the query adds 256 bytes of alignment slack; the pointer here is aligned)
    for args in _refused():
        given = args[6] if args[6] in (-1, 9) else dtype
        assert b"invalid" in go(shape=args[:6], dtype=given, ws=1 << 50), (args, given)
    for kw in (dict(sim=-1), dict(sim=2), dict(out=None), dict(qa=None)):
        assert b"invalid" in go(**kw), kw


def test_topk_orders_cosine_descending_and_mse_ascending_with_ties_by_gallery_index():
    from diffsim_amd.retrieval import topk
    m = torch.tensor([[0.1, 0.9, 0.5, 0.9, float("nan")],
                      [0.3, 0.3, 0.2, 0.8, 0.3]])
    v, i = topk(m, 3, "cosine")
    assert i.tolist() == [[1, 3, 2], [3, 0, 1]]
    assert v[0].tolist() == pytest.approx([0.9, 0.9, 0.5])
    v, i = topk(m, 5, "mse")
    assert i.tolist() == [[0, 2, 1, 3, 4], [2, 0, 1, 4, 3]]
    assert topk(m, 10, "mse")[1].shape == (2, 5)


def test_ranking_files(tmp_path):
    from diffsim_amd.retrieval import write_rankings
    qa = ["/q/dir/cat.png", "/q/other/dog.JPG"]
    gb = ["/g/a.png", "/g/b.jpg", "/g/c.jpeg"]
    m = torch.tensor([[0.5, 0.25, 0.75], [0.125, 1.0, 0.5]])
    files = write_rankings(str(tmp_path / "out"), qa, gb, m, 2, "cosine", query_root="/q")
    assert [os.path.relpath(f, tmp_path / "out") for f in files] == ["dir/cat.txt", "other/dog.txt"]
    assert open(files[0]).read() == "/g/c.jpeg 0.75\n/g/a.png 0.5\n"
    assert open(files[1]).read() == "/g/b.jpg 1\n/g/c.jpeg 0.5\n"
    files = write_rankings(str(tmp_path / "out2"), qa, gb, m, 3, "mse", query_root="/q")
    assert open(files[1]).read().split("\n")[0] == "/g/a.png 0.125"


def test_ranking_names_are_relative_to_the_query_root_and_never_collide():
    from diffsim_amd.retrieval import ranking_names
    assert ranking_names(["/q/a/cat.png", "/q/b/cat.png", "/q/dog.jpg"], "/q") == ["a/cat.txt", "b/cat.txt", "dog.txt"]
    assert ranking_names(["/q/a/cat.png", "/q/b/cat.png"]) == ["a/cat.txt", "b/cat.txt"]       # root: their common folder
    with pytest.raises(ValueError):
        ranking_names(["/q/cat.png", "/q/cat.jpg"], "/q")


def test_image_walk_is_sorted_recursive_and_case_blind(tmp_path):
    from diffsim_amd.retrieval import list_images
    for rel in ("b/x.PNG", "a/z.jpg", "a/sub/y.JpEg", "c.png", "notes.txt", "a/w.gif", "d/e.jpeg"):
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")
    got = [os.path.relpath(p, tmp_path) for p in list_images(str(tmp_path))]
    assert got == ["a/sub/y.JpEg", "a/z.jpg", "b/x.PNG", "c.png", "d/e.jpeg"]


def test_retrieval_arguments_parse_and_keep_the_reference_defaults():
    from diffsim_amd.cli import arg_parse
    a = arg_parse(["--dataset", "retrieval", "--image_path", "g", "--query_path", "q", "--out_path", "o", "--topk", "5"])
    assert (a.dataset, a.image_path, a.query_path, a.out_path, a.topk) == ("retrieval", "g", "q", "o", 5)
    assert a.similarity == "mse" and a.image_size == 512 and a.seed == 2333
    assert arg_parse(["--dataset", "retrieval"]).topk == 10


def test_retrieval_refuses_more_than_one_gpu(tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "diffsim_amd", "--dataset", "retrieval", "--image_path", str(tmp_path),
                        "--query_path", str(tmp_path), "--out_path", str(tmp_path / "o"), "--ngpu", "2"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "single-GPU" in r.stderr
    r = subprocess.run([sys.executable, "-m", "diffsim_amd", "--dataset", "retrieval", "--image_path", str(tmp_path),
                        "--query_path", str(tmp_path), "--out_path", str(tmp_path / "o"), "--selftest_shard"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "selftest_shard" in r.stderr and "Traceback" not in r.stderr
