"""Similarity maps, host side (no GPU): the C ABI's two entry points, the grid orientation of SimilarityMaps, and the
--save_maps command line."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_binds_the_map_entry_points():
    hdr = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    assert re.search(r"size_t\s+dsim_pair_score_maps_workspace_bytes\s*\(\s*int n_pairs,\s*int B,\s*int H,\s*int N,\s*int D\)", hdr)
    assert re.search(r"int\s+dsim_pair_score_maps\s*\(", hdr)
    assert re.search(r"#define\s+DSIM_ABI_VERSION\s+7\b", hdr)
    from diffsim_amd import _lib
    assert _lib.ABI_VERSION == 7
    assert len(_lib.SYMBOLS["dsim_pair_score_maps_workspace_bytes"][1]) == 5
    assert len(_lib.SYMBOLS["dsim_pair_score_maps"][1]) == 19


def test_similarity_maps_are_row_major_on_the_token_grid():
    from diffsim_amd.maps import SimilarityMaps
    n, N = 3, 64
    ramp = torch.arange(N, dtype=torch.float32).expand(n, 2, N).contiguous()
    m = SimilarityMaps(torch.zeros(n), ramp, ramp + 1000)
    assert m.grid == (8, 8) and m.local.shape == (n, 2, 8, 8) and m.contrib.shape == (n, 2, 8, 8)
    h, w = m.grid
    for r in range(h):
        for c in range(w):
            assert m.local[1, 0, r, c] == r * w + c
            assert m.contrib[2, 1, r, c] == 1000 + r * w + c
    assert len(m) == 3 and m[1].local.shape == (1, 2, 8, 8)


def test_upsample_shape_and_values():
    from diffsim_amd.maps import SimilarityMaps
    lo = torch.rand(2, 2, 256)
    m = SimilarityMaps(torch.zeros(2), lo, lo * 2)
    up = m.upsample(512)
    assert up.shape == (2, 2, 512, 512)
    assert m.upsample(64, "contrib").shape == (2, 2, 64, 64)
    assert torch.allclose(SimilarityMaps(torch.zeros(1), torch.full((1, 2, 16), 0.25), torch.zeros(1, 2, 16)).upsample(32),
                          torch.full((1, 2, 32, 32), 0.25))


def test_non_square_token_counts_are_refused():
    from diffsim_amd.maps import SimilarityMaps, grid_shape
    assert grid_shape(4096) == (64, 64)
    with pytest.raises(ValueError, match="square"):
        SimilarityMaps(torch.zeros(1), torch.zeros(1, 2, 77), torch.zeros(1, 2, 77))
    with pytest.raises(ValueError):
        grid_shape(0)


def test_save_maps_parses_only_with_the_retrieval_dataset(capsys):
    from diffsim_amd.cli import arg_parse
    a = arg_parse(["--dataset", "retrieval", "--image_path", "g", "--query_path", "q", "--out_path", "o", "--save_maps"])
    assert a.save_maps is True
    assert arg_parse(["--dataset", "retrieval"]).save_maps is False
    for ds in ("cute", "nights", "sref"):
        with pytest.raises(SystemExit) as e:
            arg_parse(["--dataset", ds, "--save_maps"])
        assert e.value.code == 2
    with pytest.raises(SystemExit):
        arg_parse(["--save_maps"])                  # (the default dataset is cute)
    assert "--dataset retrieval" in capsys.readouterr().err


def test_map_files_are_named_after_the_ranking_files(tmp_path):
    import numpy as np
    from diffsim_amd.maps import SimilarityMaps, map_names, write_map_files
    from diffsim_amd.retrieval import ranking_names
    qa = ["/q/dir/cat.png", "/q/other/dog.JPG"]
    gb = ["/g/a.png", "/g/b.jpg", "/g/c.jpeg"]
    assert map_names(qa, "/q") == ["dir/cat.npz", "other/dog.npz"]
    assert [os.path.splitext(n)[0] for n in map_names(qa, "/q")] == [os.path.splitext(n)[0] for n in ranking_names(qa, "/q")]
    idx = torch.tensor([[2, 0], [1, 2]])
    lo = torch.arange(4 * 2 * 16, dtype=torch.float32).view(4, 2, 16)
    m = SimilarityMaps(torch.tensor([0.75, 0.5, 1.0, 0.25]), lo, -lo)
    files = write_map_files(str(tmp_path), qa, gb, idx, m, "/q")
    assert [os.path.relpath(f, tmp_path) for f in files] == ["dir/cat.npz", "other/dog.npz"]
    z = np.load(files[1])
    assert z["gallery"].tolist() == ["/g/b.jpg", "/g/c.jpeg"]
    assert z["score"].tolist() == [1.0, 0.25]
    assert z["local"].shape == (2, 2, 4, 4) and z["contrib"].shape == (2, 2, 4, 4)
    assert z["local"][0, 1, 1, 2] == lo[2, 1, 6]
