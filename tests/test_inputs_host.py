"""Files to latents on the host (no GPU): ``inputs.path_latents`` without the HIP VAE equals a literal loop of reference
calls -- reseed, prepare A, prepare B, noise A, noise B -- for pair rows, triplet rows and a score matrix's two one-sided calls,
for all three scorer kinds; and ``inputs.stack_rows`` lays out the engine batch row by row."""
import glob
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMGS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "g1_img_*.png")))
SIZE = 128
SEED = 2333


def _scorer(kind):
    from diffsim_amd import config as C
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.diffsim_dit import diffsim_DiT
    from diffsim_amd.diffsim_xl import diffsim_xl
    from tests._fakes import FakeVAE, FakeVAE16
    if kind == "sd15_f32":
        return DiffSim(torch.float32, "cpu", state_dict={}, vae=FakeVAE())
    if kind == "sd15_f16":
        return DiffSim(torch.float16, "cpu", state_dict={}, vae=FakeVAE16(), noise_dtype=torch.float16)
    if kind == "xl":
        return diffsim_xl(torch.float32, "cpu", state_dict={}, vae=FakeVAE())
    return diffsim_DiT(SIZE, 600, "cpu", dit_config=C.DIT_TINY, state_dict={}, vae=FakeVAE())


def _call(sc, pa, pb):
    """(latent A, latent B, noise A, noise B) of one reference call on image files pa, pb, as f32."""
    from diffsim_amd.diffsim import DiffSim, get_generator
    from diffsim_amd.diffsim_dit import diffsim_DiT
    from diffsim_amd.image import load_image, process_image
    g = get_generator(SEED, "cpu")
    if isinstance(sc, DiffSim):
        a = sc.prepare_image_latents(process_image(load_image(pa), SIZE), None, None, g).to(sc.noise_dtype)
        b = sc.prepare_image_latents(process_image(load_image(pb), SIZE), None, None, g).to(sc.noise_dtype)
        nd = sc.noise_dtype
    else:
        a = sc.prepare_image_latents(process_image(load_image(pa), SIZE), g)
        b = sc.prepare_image_latents(process_image(load_image(pb), SIZE), g)
        nd = a.dtype if isinstance(sc, diffsim_DiT) else sc.noise_dtype       # DiT: randn_tensor(dtype=latents.dtype)
    nA = torch.randn(a.shape, generator=g, dtype=nd)
    nB = torch.randn(b.shape, generator=g, dtype=nd)
    return a.float(), b.float(), nA.float(), nB.float()


KINDS = ["sd15_f32", "sd15_f16", "xl", "dit"]


def test_golden_images_are_there():
    assert len(IMGS) == 4


@pytest.mark.parametrize("kind", KINDS)
def test_pair_rows_equal_per_call_draws(kind):
    from diffsim_amd.inputs import path_latents
    sc = _scorer(kind)
    a, b, c, d = IMGS
    rows = [(a, b), (c, d), (b, a)]
    (la, lb), nA, nB = path_latents(sc, rows, (0, 1), SIZE, SEED, 2)
    assert la.dtype == lb.dtype == nA.dtype == nB.dtype == torch.float32
    for i, (pa, pb) in enumerate(rows):
        wa, wb, wnA, wnB = _call(sc, pa, pb)
        assert torch.equal(la[i:i + 1], wa) and torch.equal(lb[i:i + 1], wb)
        assert torch.equal(nA, wnA) and torch.equal(nB, wnB)


@pytest.mark.parametrize("kind", KINDS)
def test_triplet_rows_equal_the_two_calls_per_triplet(kind):
    from diffsim_amd.inputs import path_latents
    sc = _scorer(kind)
    a, b, c, d = IMGS
    rows = [(a, b, c), (d, c, a)]
    (lr, ll, lrt), nA, nB = path_latents(sc, rows, (0, 1, 1), SIZE, SEED, 1)
    for i, (pa, pb, pc) in enumerate(rows):
        wa, wb, wnA, wnB = _call(sc, pa, pb)
        _, wc, _, _ = _call(sc, pa, pc)                 # the (A, C) call: C takes B's draw
        assert torch.equal(lr[i:i + 1], wa) and torch.equal(ll[i:i + 1], wb) and torch.equal(lrt[i:i + 1], wc)
        assert torch.equal(nA, wnA) and torch.equal(nB, wnB)


@pytest.mark.parametrize("kind", KINDS)
def test_matrix_sides_equal_per_call_draws(kind):
    from diffsim_amd.inputs import path_latents
    sc = _scorer(kind)
    queries, gallery = IMGS[:3], [IMGS[3], IMGS[0]]
    (lq,), nA, _ = path_latents(sc, [(p,) for p in queries], (0,), SIZE, SEED, 2)
    (lg,), _, nB = path_latents(sc, [(p,) for p in gallery], (1,), SIZE, SEED, 2)
    for i, q in enumerate(queries):
        for j, g in enumerate(gallery):
            wa, wb, wnA, wnB = _call(sc, q, g)
            assert torch.equal(lq[i:i + 1], wa) and torch.equal(lg[j:j + 1], wb)
            assert torch.equal(nA, wnA) and torch.equal(nB, wnB)


def test_stack_rows_interleaves_columns_and_slices_per_row_noise():
    from diffsim_amd.inputs import stack_rows
    n, shp = 5, (4, 3, 3)
    cols = [torch.randn(n, *shp, dtype=torch.float16), torch.randn(n, *shp), torch.randn(n, *shp)]
    shared, per_row = torch.randn(1, *shp), torch.randn(n, *shp)
    lat, nz = stack_rows(cols, [shared, per_row, shared], 1, 4)
    assert lat.dtype == torch.float32 and lat.shape == (9, *shp) and nz.shape == (9, *shp)
    for r in range(3):
        for c in range(3):
            assert torch.equal(lat[3 * r + c], cols[c][1 + r].float())
        assert torch.equal(nz[3 * r], shared[0]) and torch.equal(nz[3 * r + 2], shared[0])
        assert torch.equal(nz[3 * r + 1], per_row[1 + r])
    # one row: a (1, ...) noise is that row's either way
    lat, nz = stack_rows([cols[1][:1]], [per_row[2:3]], 0, 1)
    assert torch.equal(lat, cols[1][:1]) and torch.equal(nz, per_row[2:3])
