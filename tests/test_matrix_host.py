"""Score matrices, host side (no GPU): the C ABI's two entry points, the ranking rules and files, the image walk and the
--dataset retrieval command line."""
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
