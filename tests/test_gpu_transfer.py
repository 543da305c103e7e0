"""Region transfer on the GPU (csrc/transfer.hip behind dsim_pair_region_transfer; engine.pair_region_transfer, transfer.py, the
scorers' exemplar_region_score / transferred_region, harness.score_path_triplets(exemplar=), --transfer_masks), through the C ABI,
against the float64 restatement and per-entry bound of tests/_transfer64.py.

Inputs are tests/_align64.py's: 4 images, pairs (0, 1), (2, 0), (3, 1), ordinary logits and logits scaled by 14, its shapes with
their dtypes.  Each case's features, float64 reference and kernel outputs are computed once (_case) and shared by the checks.  The
gate is the bound, entry by entry, in both families; DSIM_TRANSFER_LOG=<file> appends each case's largest err / bound ratio there.
The largest ratios of the first MI355X run: see TRANSFER_FIRST_RUN below (recorded, not used: no bound is multiplied by a factor
found afterwards)."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import _align64 as A
from tests import _transfer64 as T

pytestmark = pytest.mark.gpu

B = A.B
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSFER_LOG = os.environ.get("DSIM_TRANSFER_LOG")
# first MI355X run, largest err / bound over all cases, the random-byte and 0 / 255 weight sets and both families, per dtype:
# fp32 0.019 at (49, 2, 16) ordinary bytes, bf16 0.020 at (49, 2, 16) ordinary binary, fp16 0.019 at (49, 2, 16) ordinary bytes
TRANSFER_FIRST_RUN = {"float32": 0.019, "bfloat16": 0.020, "float16": 0.019}

CASES = [(N, H, D, dt) for (N, H, D), dts in A.SHAPES.items() for dt in dts]
IDS = [f"{N}-{H}-{D}-{str(dt)[6:]}" for N, H, D, dt in CASES]
FAMILIES = {"ordinary": 1.0, "scaled": 14.0}
SETS = ("bytes", "binary", "full", "onehot")
SENTINEL = -7.0


def _idx(xs):
    return torch.tensor(list(xs), dtype=torch.int32).cuda()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _onehot_token(image, N):
    return (7 * image + 3) % N


def call(q, k, w, ia, ib, H, directions=3, ws_bytes=None, n_pairs=None, D=None, dtype=None, null=()):
    """dsim_pair_region_transfer through the C ABI on device tensors; (rc, mass (n, 2, N), status (n,)) with the outputs pre-filled
    with SENTINEL.  n_pairs, D, dtype, ws_bytes, null (names of pointers passed as NULL): what a refusal test overrides."""
    from diffsim_amd import _lib
    from diffsim_amd.engine import _TORCH2DSIM
    L = _lib.lib()
    n, (n_feat, Bc, N, HD) = ia.numel(), q.shape
    Dq = HD // H
    mass = torch.full((n, 2, N), SENTINEL, device="cuda")
    status = torch.full((n,), int(SENTINEL), dtype=torch.int32, device="cuda")
    need = int(L.dsim_pair_region_transfer_workspace_bytes(n_feat, n, Bc, H, N, Dq))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    rc = L.dsim_pair_region_transfer(_p(q), _p(k), None if "weights" in null else _p(w), n_feat, _p(ia), _p(ib),
                                     n if n_pairs is None else n_pairs, Bc, H, N, Dq if D is None else D,
                                     _TORCH2DSIM[q.dtype] if dtype is None else dtype, directions, None if "mass" in null else _p(mass),
                                     _p(status), _p(ws), need if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    return rc, mass, status


def _weight_sets(N, seed):
    """(len(SETS), 4, N) uint8: bytes uniform in 0 .. 255, 0 / 255 masks, every byte 255, one token of 255 per image"""
    onehot = torch.zeros(4, N, dtype=torch.uint8)
    for i in range(4):
        onehot[i, _onehot_token(i, N)] = 255
    return torch.stack([T.random_bytes(4, N, seed), T.binary_bytes(4, N, seed + 1), torch.full((4, N), 255, dtype=torch.uint8), onehot])


@functools.lru_cache(maxsize=None)
def _case(N, H, D, dtype, family):
    """One case, computed once: q, k on the device, the weight sets, per set the float64 mass and bound and the kernel's mass, all
    [set][pair][2][N] on the CPU"""
    q, k = A.feats(4, 11 + N + D, dtype, N, H, D, logit_scale=FAMILIES[family])
    sets = _weight_sets(N, 100 + N)
    ref, bound = T.mass64(q, k, sets, A.PAIRS, H)
    qc, kc = q.cuda(), k.cuda()
    ia, ib = _idx(p[0] for p in A.PAIRS), _idx(p[1] for p in A.PAIRS)
    got = []
    for w in sets:
        rc, mass, status = call(qc, kc, w.cuda(), ia, ib, H)
        assert rc == 0 and status.tolist() == [0] * len(A.PAIRS)
        got.append(mass.cpu().double())
    return {"q": qc, "k": kc, "ia": ia, "ib": ib, "sets": sets, "ref": ref, "bound": bound, "got": torch.stack(got)}


# ---- 1. float64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("N,H,D,dtype", CASES, ids=IDS)
def test_both_directions_stay_within_the_float64_bound(N, H, D, dtype, family):
    c = _case(N, H, D, dtype, family)
    for s, name in enumerate(SETS[:2]):
        got, ref, bound = c["got"][s], c["ref"][s], c["bound"][s]
        assert torch.isfinite(got).all() and got.min() >= 0 and got.max() <= 1 + 1e-6
        ratio = ((got - ref).abs() / bound).max().item()
        print(f"transfer {N}-{H}-{D} {str(dtype)[6:]} {family} {name}: largest err / bound = {ratio:.4f} (bound up to {bound.max():.3e})")
        if TRANSFER_LOG:
            with open(TRANSFER_LOG, "a") as f:
                f.write(json.dumps({"N": N, "H": H, "D": D, "dtype": str(dtype)[6:], "family": family, "set": name, "ratio": ratio}) + "\n")
        assert ratio <= 1.0, (name, ratio)


# ---- 2. known values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("N,H,D,dtype", CASES, ids=IDS)
def test_full_weights_give_one_and_one_hot_weights_give_the_attention_column(N, H, D, dtype, family):
    from diffsim_amd import engine
    c = _case(N, H, D, dtype, family)
    full, fb = c["got"][2], c["bound"][2]
    assert bool(((full - 1).abs() <= fb).all()), ((full - 1).abs() / fb).max().item()
    # one token of 255 in the key image: the mass is that column of Pm, which pair_align returns
    attn = engine.pair_align(c["q"], c["k"], c["ia"], c["ib"], H, return_attention=True)[3].cpu().double()
    _pm, ab = A.align64(c["q"].cpu(), c["k"].cpu(), A.PAIRS, H)
    one, ob = c["got"][3], c["bound"][3]
    for p, (a, b) in enumerate(A.PAIRS):
        for d, key_image in enumerate((b, a)):
            j = _onehot_token(key_image, N)
            err = (one[p, d] - attn[p, d, :, j]).abs()
            assert bool((err <= ob[p, d] + ab[p, d, :, j]).all()), (p, d, (err / (ob[p, d] + ab[p, d, :, j])).max().item())


# ---- 3. invariants under torch.equal ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,D,dtype", CASES, ids=IDS)
def test_repeat_alone_directions_and_other_images_weights(N, H, D, dtype):
    c = _case(N, H, D, dtype, "ordinary")
    q, k, ia, ib = c["q"], c["k"], c["ia"], c["ib"]
    w = c["sets"][0].cuda()
    rc, both, _ = call(q, k, w, ia, ib, H)
    assert rc == 0 and torch.equal(both.cpu().double(), c["got"][0])                 # a repeated call: the same bits
    for p in range(len(A.PAIRS)):                                                     # each pair alone == inside the batch
        rc, one, st = call(q, k, w, ia[p:p + 1].clone(), ib[p:p + 1].clone(), H)
        assert rc == 0 and st.tolist() == [0] and torch.equal(one[0], both[p]), p
    for directions, kept, other in ((1, 0, 1), (2, 1, 0)):                            # one direction: its rows, the others untouched
        rc, part, st = call(q, k, w, ia, ib, H, directions=directions)
        assert rc == 0 and st.tolist() == [0] * len(A.PAIRS)
        assert torch.equal(part[:, kept], both[:, kept]) and bool((part[:, other] == SENTINEL).all()), directions
    # the weights of an image that is not the row's key image change nothing: image 3 is the key image of row [2][1] alone (pair
    # (3, 1), direction 1), image 2 of row [1][1] alone (pair (2, 0))
    for image, row in ((3, (2, 1)), (2, (1, 1))):
        w2 = w.clone()
        w2[image] = 255 - w2[image]
        rc, moved, _ = call(q, k, w2, ia, ib, H)
        same = torch.ones(len(A.PAIRS), 2, dtype=torch.bool)
        same[row] = False
        assert rc == 0 and torch.equal(moved[same], both[same]) and not torch.equal(moved[row], both[row]), image
    # the Python entry point: the same bits, NaN in the rows not asked for
    from diffsim_amd import engine
    assert torch.equal(engine.pair_region_transfer(q, k, w, ia, ib, H), both)
    py2, st = engine.pair_region_transfer(q, k, w, ia, ib, H, directions=2, return_status=True)
    assert torch.equal(py2[:, 1], both[:, 1]) and bool(torch.isnan(py2[:, 0]).all()) and st.tolist() == [0] * len(A.PAIRS)


# ---- 4. non-finite features ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,D,dtype", [(49, 2, 16, torch.float32), (256, 8, 160, torch.bfloat16), (196, 8, 72, torch.float16)], ids=str)
def test_a_nan_in_one_images_k_is_reported_on_its_pairs_only(N, H, D, dtype):
    c = _case(N, H, D, dtype, "ordinary")
    w = c["sets"][0].cuda()
    k = c["k"].clone()
    k[2, 1, N // 2, 3] = float("nan")                     # image 2 is in pair 1 = (2, 0) alone, as the key image of its direction 1
    rc, mass, status = call(c["q"], k, w, c["ia"], c["ib"], H)
    assert rc == 0 and status.tolist() == [0, 1, 0]
    clean = c["got"][0]
    assert torch.equal(mass[[0, 2]].cpu().double(), clean[[0, 2]]) and torch.equal(mass[1, 0].cpu().double(), clean[1, 0])
    assert bool(torch.isnan(mass[1, 1]).all())


# ---- 5. refusals before enqueue -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    from diffsim_amd import _lib
    L = _lib.lib()
    N, H, D = 49, 2, 16
    c = _case(N, H, D, torch.float32, "ordinary")
    q, k, ia, ib = c["q"], c["k"], c["ia"], c["ib"]
    w = c["sets"][0].cuda()
    wsb = L.dsim_pair_region_transfer_workspace_bytes
    assert wsb(4, 3, B, H, N, D) > 0
    for shape in ((4, 3, B, H, N, 24), (4, 0, B, H, N, D), (0, 3, B, H, N, D)):
        assert wsb(*shape) == 0, shape
    for kw, text in ((dict(D=24), b"invalid"), (dict(dtype=7), b"invalid"), (dict(n_pairs=0), b"invalid"), (dict(directions=0), b"invalid"),
                     (dict(directions=4), b"invalid"), (dict(null=("weights",)), b"invalid"), (dict(ws_bytes=256), b"workspace")):
        rc, mass, status = call(q, k, w, ia, ib, H, **kw)
        assert rc != 0 and text in L.dsim_strerror(rc).lower(), (kw, rc)
        assert bool((mass == SENTINEL).all()) and bool((status == int(SENTINEL)).all()), kw
    rc, _mass, status = call(q, k, w, ia, ib, H, null=("mass",))
    assert rc != 0 and b"invalid" in L.dsim_strerror(rc).lower() and bool((status == int(SENTINEL)).all())


# ---- 6. planted permutations ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,D,dtype", [(N, H, D, dt) for (N, H, D) in A.PLANTED for dt in A.SHAPES[(N, H, D)]],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_a_planted_permutation_carries_the_mask_across(N, H, D, dtype):
    """Image 1's rows are image 0's permuted by pi (tests/test_transfer_host.py: every on-token's image has mass >= 0.75, every other
    <= 0.25): the transferred hard mask of image 1 is the exemplar's mask permuted by pi, and the guide's score is the region score
    with (mask, mask[pi^-1]) handed in, bit for bit."""
    from diffsim_amd import engine
    from diffsim_amd.transfer import ExemplarGuide
    q, k, pi = A.planted(3, dtype, N, H, D, A.PLANTED[(N, H, D)])
    g = torch.Generator().manual_seed(17)
    m0 = torch.zeros(N, dtype=torch.bool)
    m0[torch.randperm(N, generator=g)[:N // 2]] = True
    want = torch.zeros(N, dtype=torch.bool)
    want[pi] = m0
    pinv = torch.empty_like(pi)
    pinv[pi] = torch.arange(N)
    assert torch.equal(want, m0[pinv])
    rows = torch.stack([m0, torch.ones(N, dtype=torch.bool)]).cuda()
    ia, ib = _idx([0]), _idx([1])
    guide = ExemplarGuide()
    out, mass = guide.regions(q.cuda(), k.cuda(), H, rows, ia, ib, return_mass=True)
    assert torch.equal(out[0].cpu(), m0) and torch.equal(out[1].cpu(), want)
    assert mass[0][want.cuda()].min().item() >= 0.74 and mass[0][~want.cuda()].max().item() <= 0.26
    assert abs(guide.on_fraction - (N // 2) / N) < 1e-12
    v = torch.randn(2, B, N, H * D, generator=g).to(dtype).cuda()
    for sim in ("cosine", "mse"):
        got = engine.pair_score_regions(q.cuda(), k.cuda(), v, out.contiguous(), ia, ib, H, sim)
        handed = engine.pair_score_regions(q.cuda(), k.cuda(), v, torch.stack([m0, m0[pinv]]).cuda(), ia, ib, H, sim)
        assert torch.equal(got, handed) and bool(torch.isfinite(got).all()), sim
    # soft: the on tokens carry 255, the others their share of the threshold
    soft = ExemplarGuide(soft=True).regions(q.cuda(), k.cuda(), H, rows.to(torch.uint8) * 255, ia, ib)
    assert soft.dtype == torch.uint8 and bool((soft[1].cpu()[want] == 255).all()) and bool((soft[1].cpu()[~want] < 255).all())


# ---- 7. end to end on the tiny graphs -----------------------------------------------------------------------------------------------------
def _scorer(kind, dtype):
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.engine import VAEEncoder
    vae = VAEEncoder(C.VAE_TINY, S.make_state_dict(C.VAE_TINY, seed=3), torch.float32)
    if kind == "sd15":
        from diffsim_amd.diffsim import DiffSim
        ctx = S.make_context(C.TINY)
        return DiffSim(torch_dtype=dtype, device="cuda", unet_config=C.TINY, state_dict=S.make_state_dict(C.TINY, seed=0), vae=vae,
                       encode_prompt=lambda p: ctx), "up_blocks", [0], "a cat"
    if kind == "xl":
        from diffsim_amd.diffsim_xl import diffsim_xl
        ctx, pooled = S.make_context(C.SDXL_TINY), S.make_pooled(C.SDXL_TINY)
        return diffsim_xl(dtype, "cuda", unet_config=C.SDXL_TINY, state_dict=S.make_state_dict(C.SDXL_TINY, seed=0), vae=vae,
                          encode_prompt=lambda p: (ctx, pooled)), "up_blocks", [0, 1, 2], "a cat"
    from diffsim_amd.diffsim_dit import diffsim_DiT
    return diffsim_DiT(128, 600, "cuda", dit_config=C.DIT_TINY, state_dict=S.make_state_dict(C.DIT_TINY, seed=0), vae=vae,
                       torch_dtype=dtype), "none", [2], None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda v: str(v)[6:])
@pytest.mark.parametrize("kind", ["sd15", "xl", "dit"])
def test_tiny_graphs_end_to_end(kind, dtype, tmp_path):
    from diffsim_amd import harness as H, regions as R, transfer as X
    from diffsim_amd.inputs import path_latents
    from tests.test_gpu_regions import _image_files, _mask_files
    sc, block, layer, prompt = _scorer(kind, dtype)
    hv = {} if kind == "sd15" else {"hip_vae": False}
    lat_layer = layer if kind != "dit" else [int(layer[0])]
    imgs, mks = _image_files(tmp_path, 4, 1), _mask_files(tmp_path, 3, 2)
    pairs = [(imgs[0], imgs[1]), (imgs[2], imgs[3]), (imgs[1], imgs[0])]
    masks_a = [mks[0], None, mks[1]]
    (latA, latB), nA, nB = path_latents(sc, pairs, (0, 1), 128, 2334, 16, **hv)
    grid = R.tap_grid(sc, sc.tap_of(block, lat_layer), latA.shape[-1])
    args = (prompt, block, lat_layer, 600)
    for sim in ("cosine", "mse"):
        # hard pairs: the exemplar route is the region score fed the regions it made
        s, regs, mass = X.score_latent_pairs_exemplar(sc, latA, latB, nA, nB, masks_a, *args, sim, return_regions=True)
        assert regs.shape == (3, 2, *grid) and regs.dtype == torch.bool and mass.shape == (3, *grid) and bool(torch.isfinite(s).all())
        assert torch.equal(s, R.score_latent_pair_regions(sc, latA, latB, nA, nB, regs[:, 0], regs[:, 1], *args, sim)), sim
        assert torch.equal(regs[:, 0].cpu(), torch.stack([R.as_token_mask(m, grid) for m in masks_a]))
        assert bool(regs[1, 1].all()) and bool((mass[1] == 1).all())                       # no exemplar mask: the other image whole
        for p in (0, 2):
            assert 0 < int(regs[p, 1].sum()) < regs[p, 1].numel() and 0 < float(mass[p].min()) and float(mass[p].max()) < 1
        full = torch.zeros(3, dtype=torch.bool, device=mass.device)
        full[1] = True
        assert torch.equal(regs[:, 1].flatten(1), X.region_of_mass(mass.flatten(1), full, 1.0))
        one = X.score_latent_pairs_exemplar(sc, latA, latB, nA, nB, masks_a, *args, sim, batch_pairs=1)
        assert torch.equal(one, s)
        # soft pairs: the soft region score fed the weights it made
        ss, wts, smass = X.score_latent_pairs_exemplar(sc, latA, latB, nA, nB, masks_a, *args, sim, soft=True, return_regions=True)
        assert wts.shape == (3, 2, *grid) and wts.dtype == torch.uint8 and bool((wts[1] == 255).all())
        assert torch.equal(ss, R.score_latent_pair_weights(sc, latA, latB, nA, nB, wts[:, 0], wts[:, 1], *args, sim)), sim
        assert torch.equal(wts[:, 0].cpu(), torch.stack([R.as_token_weights(m, grid) for m in masks_a]))
        soft_rule = X.region_of_mass(smass.flatten(1), full, 1.0, soft=True)
        assert torch.equal(wts[:, 1].flatten(1), soft_rule) and bool((soft_rule[X.region_of_mass(smass.flatten(1), full, 1.0)] == 255).all())
        assert bool((soft_rule[[0, 2]] < 255).any())
        # no mask at all: the region score with full masks
        whole = torch.ones(3, *grid, dtype=torch.bool)
        assert torch.equal(X.score_latent_pairs_exemplar(sc, latA, latB, nA, nB, None, *args, sim),
                           R.score_latent_pair_regions(sc, latA, latB, nA, nB, whole, whole, *args, sim)), sim
        # from image files: the latent route
        for i, (p, m) in enumerate(zip(pairs, masks_a)):
            got = sc.exemplar_region_score(p[0], p[1], m, 128, prompt, block, layer, 600, seed=2334, similarity=sim)
            assert got.shape == (1,) and torch.equal(got[0], s[i]), (sim, i, got, s[i])
        got = sc.exemplar_region_score(pairs[0][0], pairs[0][1], masks_a[0], 128, prompt, block, layer, 600, seed=2334, similarity=sim,
                                       soft=True)
        assert torch.equal(got[0], ss[0])
    tm, tr = sc.transferred_region(pairs[0][0], pairs[0][1], masks_a[0], 128, prompt, block, layer, 600, seed=2334)
    assert torch.equal(tm, mass[0]) and torch.equal(tr, regs[0, 1])
    # three triplets == six pairwise exemplar calls; the ref's mask alone is read
    trip = [(imgs[0], imgs[1], imgs[2], prompt), (imgs[3], imgs[2], imgs[0], prompt), (imgs[1], imgs[3], imgs[2], prompt)]
    tmasks = [mks[0], None, mks[2]]
    for soft in (False, True):
        guide = X.ExemplarGuide(1.0, soft)
        sl, sr, bad = H.score_path_triplets(sc, trip, 128, block, layer, 600, 2334, "cosine", batch_triplets=2, unet_triplets=2, masks=tmasks,
                                            exemplar=guide)
        assert bad == 0 and 0.0 < guide.on_fraction < 1.0
        for i, (t, m) in enumerate(zip(trip, tmasks)):
            wl = sc.exemplar_region_score(t[0], t[1], m, 128, prompt, block, layer, 600, seed=2334, similarity="cosine", soft=soft)
            wr = sc.exemplar_region_score(t[0], t[2], m, 128, prompt, block, layer, 600, seed=2334, similarity="cosine", soft=soft)
            assert torch.equal(wl[0], sl[i]) and torch.equal(wr[0], sr[i]), (soft, i, wl, sl[i], wr, sr[i])


# ---- 8. the command line ------------------------------------------------------------------------------------------------------------------
def _write_dit_checkpoint(root):
    """A tiny DiT checkpoint in the loader's layout: <root>/dit and <root>/vae, each a config.json and a safetensors file"""
    import dataclasses
    from safetensors.torch import save_file
    from diffsim_amd import config as C, synth as S
    os.makedirs(os.path.join(root, "dit")); os.makedirs(os.path.join(root, "vae"))
    save_file({k: v.contiguous() for k, v in S.make_state_dict(C.DIT_TINY, seed=0).items()}, os.path.join(root, "dit", "model.safetensors"))
    json.dump(dataclasses.asdict(C.DIT_TINY), open(os.path.join(root, "dit", "config.json"), "w"))
    vcfg = C.VAE_TINY
    save_file({k: v.contiguous() for k, v in S.make_state_dict(vcfg, seed=1).items()},
              os.path.join(root, "vae", "diffusion_pytorch_model.safetensors"))
    json.dump({"in_channels": 3, "latent_channels": 4, "block_out_channels": list(vcfg.block_out_channels), "layers_per_block": 2,
               "norm_num_groups": 32, "scaling_factor": 0.18215}, open(os.path.join(root, "vae", "config.json"), "w"))


def test_the_command_line_transfers_the_reference_masks(tmp_path):
    from PIL import Image
    from tests.test_gpu_regions import _image_files, _mask_files
    ckpt = str(tmp_path / "ckpt")
    _write_dit_checkpoint(ckpt)
    imgs, mks = _image_files(tmp_path, 4, 1), _mask_files(tmp_path, 3, 2)
    tree, mtree = tmp_path / "cute", tmp_path / "masks"
    n = 0
    for inst in ("i0", "i1"):
        d, md = tree / "cat" / inst / "light0", mtree / "cat" / inst / "light0"
        d.mkdir(parents=True); md.mkdir(parents=True)
        for j in range(2):
            Image.open(imgs[n]).save(d / f"{j}.png")
            if n < 3:                                               # one image has no mask file
                Image.open(mks[n]).save(md / f"{j}.png")
            n += 1
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "diffsim_amd", "--metric", "dit", "--dataset", "cute", "--model_path", ckpt, "--image_path",
                        str(tree), "--mask_path", str(mtree), "--transfer_masks", "--transfer_threshold", "1.0", "--image_size", "128",
                        "--target_layer", "2", "--target_step", "600", "--similarity", "cosine", "--dtype", "fp32", "--decode_procs", "0",
                        "--batch", "4"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert "Exemplar-guided regions:" in out and "reference image(s) without a mask file" in out, out
    assert "Total comparisons: 20" in out and "Mean share of tokens on:" in out, out
    share = float(out.split("Mean share of tokens on:")[1].split("%")[0])
    assert 0.0 < share <= 100.0
