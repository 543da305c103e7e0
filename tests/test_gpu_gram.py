"""The gram metric on the GPU: the VGG executor, its ReLU / pool kernels and the Gram rows (csrc/vgg.hip), and the scorer and command
line on top (diffsim_amd/gram.py), against the float64 restatement tests/_gram64.py, which tests/test_gram_host.py pins to the
reference's own numbers.

Gates.
  * executor, f32: max |err| <= 2e-4 max |ref| (the project's q/k/v gate, tests/test_gpu_dit.py).  16-bit: the relative RMS error is at
    most twice that of the SAME restatement run by torch natively in that type on the CPU, computed in the test.
  * ReLU and ReLU + pool: torch.equal.
  * Gram rows: per entry 2 (P + 1) 2^-24 sum_p |X[p][r] X[p][c]| -- products of 16-bit values are exact in f32, the sum is f32 in some
    order; no fitted constant.  The stats' sum of squares within 1e-5 relative.
  * scores: f32 within 1e-4 relative of float64; 16-bit within twice the torch-16-bit restatement's error plus 1e-6.
Every test prints its figures before it asserts: the executor's ratio (kernel RMS error / torch's own 16-bit RMS error), the Gram rows'
measured / bound, the scores' worst error beside torch's own, score(A, A) - 1 and the matrix-cell gap.
Measured on an MI355X.  Executor, kernel RMS error / torch's own: bf16 0.97 and 0.95, fp16 0.96 and 0.95 (largest ratio 0.97); fp32 max
error 1.1e-5 against a bound of 1.7e-3.  Gram rows, measured / bound: at most 0.041 at P >= 108 and 0.24 at P = 1 in f32 (one rounded
product against a bound of two roundings); the stats' sum of squares within 9.3e-7.  Scores: bf16 worst error 5.4e-5 (last row) and
1.7e-5 (full) beside torch's own 4.5e-5 and 2.4e-5; score(A, A) - 1 at most 1.2e-7.  Matrix cell against the pair score: last row
3.6e-7, full 1.8e-7 (2.1e-6 with dsim_feature_matrix's own 16 384-element chains).  The chunked feature matrix on one-sign features of
L = 40 000: 1.5e-7 relative in f32 against the plain call's 1.8e-6.
"""
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from diffsim_amd import _lib
from tests import _gram64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
IDS = ["bf16", "fp16", "fp32"]


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


def neutral(sd, plan):
    from diffsim_amd.gram import neutral_state_dict
    return neutral_state_dict(sd, plan)


# ---- 1. the executor against float64 ------------------------------------------------------------------------------------------------
_EXEC = {}


def _exec_case(n, H, W):
    """pixels, the float64 features (channel-last) and the torch-16-bit restatement's relative RMS errors, once per shape"""
    key = (n, H, W)
    if key not in _EXEC:
        sd = R.he_state_dict(R.SMALL_PLAN, seed=5)
        pix = torch.randn(n, 3, H, W, generator=torch.Generator().manual_seed(100 + H)) * 1.1
        ref = R.features(pix, sd, R.SMALL_PLAN)
        rms = float(ref.pow(2).mean().sqrt())
        native = {}
        for dt in (torch.bfloat16, torch.float16):
            sd16 = {k: v.to(dt) for k, v in sd.items()}
            got = R.features(pix, sd16, R.SMALL_PLAN, dt).double()
            native[dt] = float((got - ref).pow(2).mean().sqrt()) / rms
        _EXEC[key] = (sd, pix, ref.permute(0, 2, 3, 1).contiguous(), rms, native)
    return _EXEC[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,H,W", [(2, 40, 56), (1, 37, 51)], ids=["2x40x56", "1x37x51"])
def test_executor_against_float64(eng, n, H, W, dtype):
    """Plan (64, 64, P, 128, 128, P, 256), He-initialised.  37 x 51 pools to 18 x 25, then 9 x 12: both pools drop a row and a column.
    Largest 16-bit ratio (kernel RMS error / torch's own) measured on an MI355X: see the printed figure."""
    sd, pix, ref, rms, native = _exec_case(n, H, W)
    e = eng.VGGEngine(R.SMALL_PLAN, neutral(sd, R.SMALL_PLAN), dtype)
    assert e.out_shape(H, W) == (H // 4, W // 4, 256)
    got = e.features(pix.cuda())
    assert got.shape == ref.shape and got.dtype == dtype
    err = got.double().cpu() - ref
    if dtype == torch.float32:
        m, bound = float(err.abs().max()), 2e-4 * float(ref.abs().max())
        print(f"executor fp32 {n}x{H}x{W}: max err {m:.3e}, bound {bound:.3e}")
        assert m <= bound
    else:
        r = float(err.pow(2).mean().sqrt()) / rms
        print(f"executor {dtype} {n}x{H}x{W}: rel RMS {r:.3e}, torch's own {native[dtype]:.3e}, ratio {r / native[dtype]:.3f}")
        assert r <= 2.0 * native[dtype]


# ---- 2. ReLU and ReLU + pool alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("H,W", [(7, 9), (1, 2), (2, 2), (8, 6)], ids=["7x9", "1x2", "2x2", "8x6"])
def test_relu_and_pool_bit_exact(eng, H, W, dtype):
    """64 channels, odd extents: against torch with torch.equal.  1 x 2 has no pooled output (the executor refuses it; the op too) and
    checks the ReLU alone.  The dropped odd row / column is poisoned with NaN: a kernel that read it would spread it."""
    x = (torch.randn(2, H, W, 64, generator=torch.Generator().manual_seed(H * 16 + W)) * 2).to(dtype)
    want_relu = torch.relu(x.float()).to(dtype)
    assert torch.equal(eng.op_relu(x.cuda()).cpu(), want_relu)
    if H < 2:
        with pytest.raises(_lib.DsimError):
            eng.op_relu_pool2(x.cuda())
        return
    xp = x.clone()
    if H % 2:
        xp[:, H - 1] = float("nan")
    if W % 2:
        xp[:, :, W - 1] = float("nan")
    want = torch.nn.functional.max_pool2d(torch.relu(x.float()).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).to(dtype)
    got = eng.op_relu_pool2(xp.cuda()).cpu()
    assert got.shape == (2, H // 2, W // 2, 64)
    assert torch.equal(got, want)


def test_relu_and_pool_propagate_nan(eng):
    x = torch.randn(1, 4, 4, 8)
    x[0, 1, 1, 3] = float("nan")
    assert bool(torch.isnan(eng.op_relu(x.cuda())[0, 1, 1, 3]))
    p = eng.op_relu_pool2(x.cuda()).cpu()
    assert bool(torch.isnan(p[0, 0, 0, 3])) and int(torch.isnan(p).sum()) == 1


# ---- 3. Gram rows against float64 ---------------------------------------------------------------------------------------------------
def _gram_case(P, Cc, dtype, seed=7, n=3):
    x = (torch.randn(n, P, Cc, generator=torch.Generator().manual_seed(seed + P)) * 1.5 + 0.25).to(dtype)
    xd = x.double()
    want = xd.transpose(1, 2) @ xd                                   # [n][C][C]
    bound = 2.0 * (P + 1) * 2.0 ** -24 * (xd.abs().transpose(1, 2) @ xd.abs())
    return x, want, bound


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("P,Cc", [(108, 256), (1024, 512), (1, 64)], ids=["108x256", "1024x512", "1x64"])
def test_gram_rows_against_float64(eng, P, Cc, dtype):
    """Row -1 alone (the vector kernel) and all rows (the matrix cores in the 16-bit types); P = 1024 folds two partials, P = 108 ends
    inside a stage, P = 1 is one position.  measured / bound is printed; the largest seen on an MI355X is recorded in the summary."""
    x, want, bound = _gram_case(P, Cc, dtype)
    xg = x.cuda()
    for row0, n_rows in ((Cc - 1, 1), (0, Cc)):
        out, stats = eng.gram_rows(xg, row0, n_rows)
        assert out.shape == (3, n_rows, Cc) and out.dtype == torch.float32 and stats.shape == (3, 4)
        w, b = want[:, row0:row0 + n_rows], bound[:, row0:row0 + n_rows]
        err = (out.double().cpu() - w).abs()
        ratio = float((err / b.clamp_min(1e-300)).max())
        ss = (w ** 2).sum((1, 2))
        ss_err = float(((stats[:, 0].double().cpu() - ss).abs() / ss).max())
        print(f"gram rows P {P} C {Cc} {dtype} rows [{row0}, {row0 + n_rows}): measured / bound {ratio:.3f}, ss rel err {ss_err:.2e}")
        assert bool((err <= b).all()), ratio
        assert ss_err <= 1e-5
        assert torch.equal(stats[:, 1].cpu(), out.amin((1, 2)).cpu()) and torch.equal(stats[:, 2].cpu(), out.amax((1, 2)).cpu())
        assert bool((stats[:, 3] == 0).all())
        out2, stats2 = eng.gram_rows(xg, row0, n_rows)
        assert torch.equal(out, out2) and torch.equal(stats, stats2)                    # twice the same call: equal bits
        for i in range(3):                                                              # each image alone: its rows in the batch
            oi, si = eng.gram_rows(xg[i:i + 1].contiguous(), row0, n_rows)
            assert torch.equal(oi[0], out[i]) and torch.equal(si[0], stats[i]), i
    last, _ = eng.gram_rows(xg, -1, 1)
    assert torch.equal(last, eng.gram_rows(xg, Cc - 1, 1)[0])


# ---- 3b. the feature matrix in shorter partial sums ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_chunked_feature_matrix(eng, dtype):
    """dsim_feature_matrix_chunked on 3 x 5 one-sign features of L = 40 000 (no multiple of a chunk): k_chunk = 16384 and k_chunk >= L
    are dsim_feature_matrix bit for bit; 1024 holds the same bound against float64 (tests/test_gpu_feats.py BOUND: 4e-3 / 5e-4
    absolute in the 16-bit types, 1e-5 relative in f32), deterministic, a cell alone equal to its place in the matrix; a k_chunk
    outside the list is refused."""
    L, na, nb = 40000, 3, 5
    g = torch.Generator().manual_seed(77)
    mk = lambda n: (torch.rand(n, L, generator=g) * torch.linspace(0.2, 1.0, L) + 0.05 * torch.rand(n, 1, generator=g)).to(dtype)
    xa, xb = mk(na), mk(nb)
    st = lambda x: torch.cat([(x.double() ** 2).sum(1, keepdim=True).float(), torch.zeros(x.shape[0], 3)], 1).cuda()
    fa, fb = (xa.cuda(), st(xa)), (xb.cuda(), st(xb))
    want = torch.stack([torch.stack([R.cosine(a.double(), b.double()) for b in xb]) for a in xa])
    plain = eng.feature_matrix(fa, fb)
    assert torch.equal(eng.feature_matrix(fa, fb, k_chunk=16384), plain)
    m, status = eng.feature_matrix(fa, fb, return_status=True, k_chunk=1024)
    err = (m.double().cpu() - want).abs()
    if dtype == torch.float32:
        err = err / want.abs()
    bound = {torch.bfloat16: 4e-3, torch.float16: 5e-4, torch.float32: 1e-5}[dtype]
    print(f"chunked feature matrix {dtype}: err {float(err.max()):.3e} (plain call {float((plain.double().cpu() - want).abs().max()):.3e}), bound {bound:.1e}")
    assert float(err.max()) <= bound and not bool(status.any())
    assert torch.equal(m, eng.feature_matrix(fa, fb, k_chunk=1024))
    one = eng.feature_matrix((fa[0][2:3].contiguous(), fa[1][2:3].contiguous()), (fb[0][4:5].contiguous(), fb[1][4:5].contiguous()), k_chunk=1024)
    assert torch.equal(one[0, 0], m[2, 4])
    for bad in (1000, 32, 32768):
        with pytest.raises(_lib.DsimError):
            eng.feature_matrix(fa, fb, k_chunk=bad)


# ---- 5. refusals enqueue nothing ----------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(eng):
    sd = R.he_state_dict(R.SMALL_PLAN, seed=5)
    nsd = neutral(sd, R.SMALL_PLAN)
    for bad in (("P", 64), (64, "P"), (64, "P", "P", 64), (12,), (64, -3, 64), tuple([64] * 40)):
        with pytest.raises(_lib.DsimError):
            eng.VGGEngine(bad, nsd, torch.float32)
    with pytest.raises(_lib.DsimError):
        eng.VGGEngine(R.SMALL_PLAN, nsd, torch.float64)                  # a dtype outside the list
    with pytest.raises(_lib.DsimError):
        eng.VGGEngine(R.SMALL_PLAN, {k: v for k, v in nsd.items() if k != "convs.3.bias"}, torch.float32)      # a missing parameter
    e = eng.VGGEngine(R.SMALL_PLAN, nsd, torch.bfloat16)
    L = _lib.lib()
    pix = torch.randn(1, 3, 8, 12).cuda()
    out = torch.full((1, 2, 3, 256), -7.0, dtype=torch.bfloat16).cuda()
    need = e.workspace_bytes(1, 8, 12)
    assert need > 0 and e.workspace_bytes(0, 8, 12) == 0 and e.workspace_bytes(1, 3, 12) == 0
    ws = torch.empty(need, dtype=torch.uint8).cuda()
    s = torch.cuda.current_stream().cuda_stream
    assert L.dsim_vgg_features(e._h, pix.data_ptr(), 0, 8, 12, out.data_ptr(), ws.data_ptr(), need, s) == -1        # n < 1
    assert L.dsim_vgg_features(e._h, pix.data_ptr(), 1, 3, 12, out.data_ptr(), ws.data_ptr(), need, s) == -1        # smaller than the pools
    assert L.dsim_vgg_features(e._h, pix.data_ptr(), 1, 8, 12, out.data_ptr(), ws.data_ptr(), need - 257, s) == -3  # a short workspace
    with pytest.raises(_lib.DsimError):
        e.features(torch.randn(1, 3, 8, 12).double().cuda())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    # the Gram rows: C % 8, a row range outside the matrix, n < 1, a short workspace
    x = torch.randn(2, 10, 64).cuda()
    g = torch.full((2, 64, 64), -7.0).cuda()
    st = torch.full((2, 4), -7.0).cuda()
    for args in ((2, 10, 60, 0, 60), (2, 10, 64, 60, 8), (2, 10, 64, -1, 1), (0, 10, 64, 0, 64), (2, 0, 64, 0, 64), (2, 10, 64, 0, 0)):
        assert L.dsim_gram_rows_workspace_bytes(*args, _lib.DSIM_F32) == 0
        assert L.dsim_gram_rows(x.data_ptr(), *args, _lib.DSIM_F32, g.data_ptr(), st.data_ptr(), ws.data_ptr(), need, s) == -1
    assert L.dsim_gram_rows_workspace_bytes(2, 10, 64, 0, 64, 7) == 0
    gneed = L.dsim_gram_rows_workspace_bytes(2, 10, 64, 0, 64, _lib.DSIM_F32)
    assert L.dsim_gram_rows(x.data_ptr(), 2, 10, 64, 0, 64, _lib.DSIM_F32, g.data_ptr(), st.data_ptr(), ws.data_ptr(), gneed - 257, s) == -3
    with pytest.raises(_lib.DsimError):
        eng.gram_rows(x, 60, 8)
    torch.cuda.synchronize()
    assert bool((g == -7.0).all()) and bool((st == -7.0).all())


# ---- 4. scores: files in, against float64 -------------------------------------------------------------------------------------------
SIZES = [(60, 44), (60, 44), (45, 70), (80, 50)]          # (w, h): four non-square images of three sizes; at --image_size 32 two share 43 x 32
IMG_SIZE = 32


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """four PNGs (smooth seeded noise, so that the bilinear resize has something to average) and the float64 restatement's inputs"""
    root = tmp_path_factory.mktemp("gram_imgs")
    paths = []
    for i, (w, h) in enumerate(SIZES):
        rng = np.random.default_rng(40 + i)
        small = rng.integers(0, 256, (h // 4 + 1, w // 4 + 1, 3), dtype=np.uint8)
        im = Image.fromarray(small).resize((w, h), Image.BICUBIC)
        p = str(root / f"im{i}.png")
        im.save(p)
        paths.append(p)
    return paths


def _pixels64(path):
    """vgg_gram.load_image restated: RGB, Resize(32) by the size rule with PIL's bilinear, ToTensor, Normalize -- in float64"""
    im = Image.open(path).convert("RGB")
    w, h = im.size
    if min(w, h) != IMG_SIZE:
        im = im.resize((int(IMG_SIZE * w / h), IMG_SIZE) if h <= w else (IMG_SIZE, int(IMG_SIZE * h / w)), Image.BILINEAR)
    return R.normalise(np.asarray(im))


_SCORES = {}


def _score_refs(files):
    """float64 scores of every ordered pair and mode, and the torch-16-bit restatement's largest error per (dtype, mode)"""
    if not _SCORES:
        sd = R.he_state_dict(R.SMALL_PLAN, seed=9)
        px = [_pixels64(p) for p in files]
        want, native = {}, {}
        for full in (False, True):
            for i in range(4):
                for j in range(4):
                    want[(i, j, full)] = float(R.similarity(px[i], px[j], sd, R.SMALL_PLAN, full))
            for dt in (torch.bfloat16, torch.float16):
                sd16 = {k: v.to(dt) for k, v in sd.items()}
                native[(dt, full)] = max(abs(float(R.similarity(px[i], px[j], sd16, R.SMALL_PLAN, full, dt)) - want[(i, j, full)])
                                         for i in range(4) for j in range(i + 1, 4))
        _SCORES.update(sd=sd, want=want, native=native)
    return _SCORES["sd"], _SCORES["want"], _SCORES["native"]


def _scorer(sd, dtype):
    from diffsim_amd.gram import VGGGram
    return VGGGram(R.SMALL_PLAN, sd, "cuda", dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scores_from_files(files, dtype):
    """gram_similarity against the restatement: f32 within 1e-4 relative; 16-bit within twice the torch-16-bit restatement's error
    (its largest over the six pairs of the mode: a single pair's can be small by chance) plus 1e-6.  Then: a mixed-size batch equals
    each pair alone bit for bit, triplets equal the pairwise calls, score(A, A) = 1 within 1e-6."""
    sd, want, native = _score_refs(files)
    sc = _scorer(sd, dtype)
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    for full in (False, True):
        worst = 0.0
        for i, j in pairs:
            s = sc.gram_similarity(files[i], files[j], IMG_SIZE, full)
            assert s.shape == (1,) and s.dtype == torch.float32
            err = abs(float(s) - want[(i, j, full)])
            worst = max(worst, err)
            if dtype == torch.float32:
                assert err <= 1e-4 * abs(want[(i, j, full)]), (i, j, full, err)
            else:
                assert err <= 2.0 * native[(dtype, full)] + 1e-6, (i, j, full, err, native[(dtype, full)])
        print(f"scores {dtype} full={full}: worst err {worst:.3e}"
              + ("" if dtype == torch.float32 else f", torch's own worst {native[(dtype, full)]:.3e}")
              + f", scores {min(want[(i, j, full)] for i, j in pairs):.4f} .. {max(want[(i, j, full)] for i, j in pairs):.4f}")
        # PIL images in: the same bits as paths in
        assert torch.equal(sc.gram_similarity(Image.open(files[0]), Image.open(files[2]), IMG_SIZE, full),
                           sc.gram_similarity(files[0], files[2], IMG_SIZE, full))
        alone = {p: sc.gram_similarity(files[p[0]], files[p[1]], IMG_SIZE, full)[0] for p in pairs + [(0, 0), (2, 2), (3, 1)]}
        batch, st = sc.score_path_pairs([(files[i], files[j]) for i, j in pairs], IMG_SIZE, full, return_status=True)
        assert not bool(st.any())
        for t, p in enumerate(pairs):
            assert torch.equal(batch[t], alone[p]), (p, full)
        trip = [(files[0], files[1], files[2], "p"), (files[3], files[1], files[0], "p"), (files[2], files[2], files[3], "p")]
        s_ab, s_ac, bad = sc.score_path_triplets(trip, IMG_SIZE, full)
        assert bad == 0
        assert torch.equal(s_ab[0], alone[(0, 1)]) and torch.equal(s_ac[0], alone[(0, 2)])
        assert torch.equal(s_ab[1], alone[(3, 1)]) and torch.equal(s_ab[2], alone[(2, 2)])
        self_err = max(abs(float(alone[(0, 0)]) - 1.0), abs(float(alone[(2, 2)]) - 1.0))
        print(f"  score(A, A) - 1: {self_err:.3e}")
        assert self_err <= 1e-6


@pytest.mark.parametrize("full", [False, True], ids=["last-row", "full"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_matrix_cells_against_pair_scores(files, dtype, full):
    """Matrix cells (engine.feature_matrix on the descriptors, in gram.MATRIX_KCHUNK-element partial sums) agree with the pair scores
    within the feature metrics' recorded gap for f32 features, 9.5e-7 (tests/test_gpu_feats.py: "a cell against its pair score 3.0e-7
    (f32 9.5e-7)").  With dsim_feature_matrix's own 16 384-element f32 chains the full descriptor (L = 65 536, every term of one sign)
    measured 2.1e-6 on an MI355X and missed the gate; the chunked call is why it holds now."""
    sd, _, _ = _score_refs(files)
    sc = _scorer(sd, dtype)
    m, nbad = sc.score_path_matrix(files[:3], files[1:], IMG_SIZE, full, return_status=True)
    cells = torch.stack([sc.gram_similarity(a, b, IMG_SIZE, full)[0] for a in files[:3] for b in files[1:]]).view(3, 3)
    gap = float((m - cells).abs().max())
    print(f"matrix cell against the pair score, {dtype} full={full}: {gap:.3e}")
    assert m.shape == (3, 3) and m.dtype == torch.float32 and nbad == 0
    assert gap <= 9.5e-7


def test_last_row_and_full_scores_differ(files):
    sd, want, _ = _score_refs(files)
    assert max(abs(want[(i, j, False)] - want[(i, j, True)]) for i in range(4) for j in range(i + 1, 4)) > 1e-3


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nan_pixel_marks_its_own_pairs_only(files, dtype):
    sd, _, _ = _score_refs(files)
    sc = _scorer(sd, dtype)
    pix = torch.randn(3, 3, 32, 43, generator=torch.Generator().manual_seed(3)).cuda()
    from diffsim_amd.engine import feature_pair_score
    ia = torch.tensor([0, 0, 1], dtype=torch.int32).cuda()
    ib = torch.tensor([1, 2, 2], dtype=torch.int32).cuda()
    for full in (False, True):
        clean = feature_pair_score(*sc.descriptors_of_pixels(pix, full), ia, ib)
        bad = pix.clone()
        bad[1, 2, 17, 5] = float("nan")
        s, st = feature_pair_score(*sc.descriptors_of_pixels(bad, full), ia, ib, return_status=True)
        assert st.tolist() == [1, 0, 1] and bool(torch.isnan(s[0])) and bool(torch.isnan(s[2]))
        assert torch.equal(s[1], clean[1])


# ---- 6. the command line, end to end ------------------------------------------------------------------------------------------------
def test_cli_sref_then_retrieval(files, tmp_path, capsys):
    from diffsim_amd import cli
    from tests.test_gram_host import _write_checkpoint
    ckpt, tree, out = str(tmp_path / "ckpt"), str(tmp_path / "styles"), str(tmp_path / "rank")
    _write_checkpoint(ckpt)
    n = 0
    for style in ("ink", "oil", "wax"):
        os.makedirs(os.path.join(tree, style))
        for j in range(2):
            Image.open(files[n % 4]).rotate(90 * (n // 4), expand=True).save(os.path.join(tree, style, f"im{j}.png"))
            n += 1
    base = ["--metric", "gram", "--model_path", ckpt, "--similarity", "cosine", "--image_size", str(IMG_SIZE), "--decode_procs", "0"]
    assert cli.main(base + ["--dataset", "sref", "--image_path", tree, "--experiments", "12", "--dtype", "bf16"]) == 0
    text = capsys.readouterr().out
    assert "last rows of the Gram matrices" in text and "Total comparisons: 12" in text and "Accuracy:" in text, text
    assert "WARNING" not in text, text
    from diffsim_amd.engine import RESIZE_COUNTS
    before = dict(RESIZE_COUNTS)                # (the counts run since the process started)
    assert cli.main(base + ["--dataset", "retrieval", "--query_path", os.path.join(tree, "ink"), "--image_path", tree, "--out_path", out,
                            "--dtype", "fp32", "--topk", "3", "--gram_full", "--gpu_resize"]) == 0
    text = capsys.readouterr().out
    assert "whole Gram matrices" in text and "Score matrix (2, 6)" in text, text
    # bilinear is not one of the device resize's filters: all 2 + 6 images are host fallbacks
    assert RESIZE_COUNTS["gpu"] == before["gpu"] and RESIZE_COUNTS["fallback"] == before["fallback"] + 8
    assert f"{RESIZE_COUNTS['gpu']} image(s) resized on the device, {RESIZE_COUNTS['fallback']} fell back to the host" in text, text
    ranked = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert ranked == ["im0.txt", "im1.txt"], ranked
    for f in ranked:
        lines = open(os.path.join(out, f)).read().splitlines()
        assert len(lines) == 3
        first = lines[0].rsplit(" ", 1)
        # the query is in the gallery: ranked first, its cell 1 within the f32 matrix cells' own bound against float64 (1e-5,
        # tests/test_gpu_feats.py BOUND) -- a cell's dot product and the norms under it are folded by different kernels
        assert first[0] == os.path.join(tree, "ink", f[:-4] + ".png") and abs(float(first[1]) - 1.0) <= 1e-5
