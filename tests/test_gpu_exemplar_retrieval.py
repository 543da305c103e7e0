"""Exemplar-guided retrieval on the GPU (retrieval.score_latent_matrix_exemplar, score_path_matrix with exemplar=, ExemplarGuide.cell_regions,
--dataset retrieval --query_mask_path --transfer_masks): a query's mask picks the region of every gallery image, one region per
cell.  The contract is the pair path's: cell (i, j) is transfer.score_latent_pairs_exemplar of the pair (latA[i], latB[j]) -- score,
transferred region and mass, bit for bit -- on tests/test_gpu_transfer.py's tiny SD1.5, SDXL and DiT graphs."""
import os
import subprocess
import sys

import pytest
import torch

from tests import _align64 as A
from tests.test_gpu_transfer import _scorer, _write_dit_checkpoint

pytestmark = pytest.mark.gpu

B = A.B
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _latents(sc, kind, tmp_path, n_a, n_b):
    from diffsim_amd.inputs import path_latents
    from tests.test_gpu_regions import _image_files
    hv = {} if kind == "sd15" else {"hip_vae": False}
    qa, gb = _image_files(tmp_path, n_a, 1), _image_files(tmp_path, n_b, 2)
    (latA,), nA, _ = path_latents(sc, [(p,) for p in qa], (0,), 128, 2334, 16, **hv)
    (latB,), _, nB = path_latents(sc, [(p,) for p in gb], (1,), 128, 2334, 16, **hv)
    return latA, latB, nA, nB


# ---- 1. the pair path, cell by cell, and two gallery chunks -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda v: str(v)[6:])
@pytest.mark.parametrize("kind", ["sd15", "xl", "dit"])
def test_the_matrix_equals_the_pair_path_cell_by_cell(kind, dtype, tmp_path):
    """Three queries -- a mask file, no mask, a full mask -- against three gallery images, hard and soft guides, cosine and mse: the
    scores, the transferred regions and the masses are the pair path's; the rows of the query without a mask and of the one with a
    full mask are the plain score matrix's (every gallery image whole, mass 1); two gallery chunks give the matrix of one."""
    from diffsim_amd import regions as R, transfer as X
    from diffsim_amd.retrieval import score_latent_matrix, score_latent_matrix_exemplar
    from tests.test_gpu_regions import _mask_files
    sc, block, layer, prompt = _scorer(kind, dtype)
    layer = layer if kind != "dit" else [int(layer[0])]
    n_a, n_b = 3, 3
    latA, latB, nA, nB = _latents(sc, kind, tmp_path, n_a, n_b)
    grid = R.tap_grid(sc, sc.tap_of(block, layer), latA.shape[-1])
    masks_a = [_mask_files(tmp_path, 1, 2)[0], None, torch.ones(grid, dtype=torch.bool)]
    args = (prompt, block, layer, 600)
    pairs = (latA.repeat_interleave(n_b, 0), latB.repeat(n_a, 1, 1, 1), nA, nB, [m for m in masks_a for _ in range(n_b)])
    for soft in (False, True):
        for sim in ("cosine", "mse"):
            guide = X.ExemplarGuide(1.0, soft)
            m, bad, regs, mass = score_latent_matrix_exemplar(sc, latA, latB, nA, nB, *args, sim, return_status=True, masks_a=masks_a,
                                                              exemplar=guide, return_regions=True)
            s, pregs, pmass = X.score_latent_pairs_exemplar(sc, *pairs, *args, sim, soft=soft, return_regions=True)
            assert bad == 0 and m.shape == (n_a, n_b) and bool(torch.isfinite(m).all())
            assert regs.shape == (n_a, n_b, *grid) and regs.dtype == (torch.uint8 if soft else torch.bool) and mass.shape == (n_a, n_b, *grid)
            assert torch.equal(m, s.view(n_a, n_b)), (soft, sim, m, s)
            assert torch.equal(regs, pregs[:, 1].view(n_a, n_b, *grid)) and torch.equal(mass, pmass.view(n_a, n_b, *grid)), (soft, sim)
            whole = 255 if soft else True
            assert bool((regs[0] == whole).any()) and not bool((regs[0] == whole).all()) and float(mass[0].max()) < 1      # the masked query: true regions
            assert bool((regs[1:] == whole).all()) and bool((mass[1:] == 1).all())
            assert 0.0 < guide.on_fraction < 1.0
            plain = score_latent_matrix(sc, latA, latB, nA, nB, *args, sim)
            assert torch.equal(m[1:], plain[1:]) and not torch.equal(m[0], plain[0]), (soft, sim, m, plain)
            assert torch.equal(score_latent_matrix_exemplar(sc, latA, latB, nA, nB, *args, sim, masks_a=masks_a, exemplar=X.ExemplarGuide(1.0, soft)), m)
            two = score_latent_matrix_exemplar(sc, latA, latB, nA, nB, *args, sim, batch=2, masks_a=masks_a, exemplar=X.ExemplarGuide(1.0, soft),
                                               return_regions=True)                                                 # two gallery chunks
            assert torch.equal(two[0], m) and torch.equal(two[1], regs) and torch.equal(two[2], mass), (soft, sim)


# ---- 2. planted permutations --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,D,dtype", [(N, H, D, dt) for (N, H, D) in A.PLANTED for dt in A.SHAPES[(N, H, D)]],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_planted_permutations_carry_the_mask_to_every_gallery_image(N, H, D, dtype):
    """Three gallery images, each the query's rows under another permutation (tests/_align64.py's planted construction and gains):
    the region of cell (0, g) is the query's mask under permutation g, bit for bit, and the cell-region matrix scores it as the
    region matrix scores the masks handed in."""
    from diffsim_amd import engine
    from diffsim_amd.transfer import ExemplarGuide
    q2, _k2, _pi = A.planted(3, dtype, N, H, D, A.PLANTED[(N, H, D)])
    x = q2[0]                                                     # (B, N, H D): the query, q = k
    g = torch.Generator().manual_seed(17)
    perms = [torch.randperm(N, generator=g) for _ in range(3)]
    ys = []
    for pi in perms:
        y = torch.empty_like(x)
        y[:, pi] = x                                              # row pi[i] of the gallery image is row i of the query
        ys.append(y)
    qa = x.unsqueeze(0).contiguous().cuda()
    qb = torch.stack(ys).contiguous().cuda()
    m0 = torch.zeros(N, dtype=torch.bool)
    m0[torch.randperm(N, generator=g)[:N // 2]] = True
    want = torch.zeros(3, N, dtype=torch.bool)
    for gi, pi in enumerate(perms):
        want[gi, pi] = m0
    assert len({tuple(w.tolist()) for w in want}) == 3
    v = torch.randn(4, B, N, H * D, generator=g).to(dtype).cuda()
    fa, fb = (qa, qa.clone(), v[:1].contiguous()), (qb, qb.clone(), v[1:].contiguous())
    guide = ExemplarGuide()
    regs, mass = guide.cell_regions(fa, fb, H, m0[None].cuda())
    assert regs.shape == (1, 3, N) and regs.dtype == torch.bool and torch.equal(regs[0].cpu(), want)
    assert mass[0][want.cuda()].min().item() >= 0.74 and mass[0][~want.cuda()].max().item() <= 0.26
    assert abs(guide.on_fraction - (N // 2) / N) < 1e-12
    for sim in ("cosine", "mse"):
        got = engine.score_matrix_cell_regions(fa, fb, m0[None].cuda(), regs.contiguous(), H, sim)
        handed = engine.score_matrix_regions(fa, fb, m0[None].cuda(), want.cuda(), H, sim)
        assert torch.equal(got, handed) and bool(torch.isfinite(got).all()), sim
    soft, _ = ExemplarGuide(soft=True).cell_regions(fa, fb, H, m0[None].to(torch.uint8).cuda() * 255)
    assert soft.dtype == torch.uint8 and bool((soft[0].cpu()[want] == 255).all()) and bool((soft[0].cpu()[~want] < 255).all())


# ---- 3. the command line ------------------------------------------------------------------------------------------------------------------
def test_the_command_line_ranks_by_the_transferred_regions(tmp_path):
    """--dataset retrieval --query_mask_path --transfer_masks --save_transfer on a tiny DiT checkpoint and image tree (one query has
    no mask file): exit 0, one ranking per query, a .transfer.npz beside each with region and mass (k, h, w), the mean share printed;
    a misuse exits with 2 and names the flag."""
    import numpy as np
    from PIL import Image
    from tests.test_gpu_regions import _image_files, _mask_files
    ckpt = str(tmp_path / "ckpt")
    _write_dit_checkpoint(ckpt)
    qdir, gdir, qm, out = (tmp_path / d for d in ("q", "g", "qm", "out"))
    for d in (qdir, gdir, qm):
        d.mkdir()
    _image_files(qdir, 2, 11), _image_files(gdir, 4, 12)
    Image.open(_mask_files(tmp_path, 1, 2)[0]).save(qm / "img11_0.png")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "diffsim_amd", "--metric", "dit", "--dataset", "retrieval", "--model_path", ckpt, "--query_path", str(qdir),
            "--image_path", str(gdir), "--out_path", str(out), "--image_size", "128", "--target_layer", "2", "--target_step", "600",
            "--similarity", "cosine", "--dtype", "fp32", "--decode_procs", "0", "--topk", "3"]
    r = subprocess.run(base + ["--query_mask_path", str(qm), "--transfer_masks", "--transfer_threshold", "1.0", "--save_transfer"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    text = r.stdout
    assert "Exemplar-guided retrieval:" in text and "1 query image(s) without a mask file" in text, text
    assert "Mean share of tokens on:" in text and "Transferred regions" in text, text
    share = float(text.split("Mean share of tokens on:")[1].split("%")[0])
    assert 0.0 < share < 100.0
    for name in ("img11_0", "img11_1"):
        rank = open(out / f"{name}.txt").read().splitlines()
        assert len(rank) == 3
        z = np.load(out / f"{name}.transfer.npz")
        assert set(z.files) == {"gallery", "region", "mass"}
        k, h, w = z["region"].shape
        assert k == 3 and h == w and z["region"].dtype == np.bool_ and z["mass"].shape == (3, h, w) and z["mass"].dtype == np.float32
        assert z["gallery"].tolist() == [l.split()[0] for l in rank]
    assert 0 < np.load(out / "img11_0.transfer.npz")["region"].sum() < 3 * h * w
    assert np.load(out / "img11_1.transfer.npz")["region"].all()                          # no mask file: every gallery image whole
    for extra, named in ((["--query_mask_path", str(qm), "--transfer_masks", "--gallery_mask_path", str(qm)], "--transfer_masks"),
                         (["--mask_path", str(qm), "--transfer_masks"], "--query_mask_path")):
        r = subprocess.run(base + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and named in r.stderr and "--transfer_masks" in r.stderr, r.stderr
