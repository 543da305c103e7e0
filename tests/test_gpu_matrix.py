"""Score matrices (dsim_score_matrix / engine.score_matrix / retrieval.score_latent_matrix): every image of set A against every
image of set B, each image's self-attention computed once.  Checked against the reference's tail arithmetic restated in float64
torch (/root/reference/diffsim/diffsim.py:177-197) and against the pair path (engine.pair_score) on the same features."""
import pytest
import torch

from tests._tail64 import matrix64

pytestmark = pytest.mark.gpu

B = 2


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


def _tail64(fa, fb, H, sim, out_dtype):
    """float64 SDPAs on the rounded operands, their outputs rounded to the pipeline dtype, cosine / mse in float64:
    the (n_a, n_b) matrix of diffsim.py:177-197 over every (a, b) (tests/_tail64.py, query-chunked)"""
    return matrix64(fa, fb, H, sim, out_dtype)


def _feats(n, seed, dtype, N, H, D, logit_scale=1.0, correlate=0.0, base=None):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(n, B, N, H * D, generator=g) for _ in range(3))
    if correlate:                   # images that resemble a common base: scores away from zero
        base = base if base is not None else tuple(torch.randn(1, B, N, H * D, generator=g) for _ in range(3))
        q, k, v = (correlate * b + (1 - correlate) * t for b, t in zip(base, (q, k, v)))
    q = q * logit_scale
    return tuple(t.to(dtype).cuda().contiguous() for t in (q, k, v))


def _pair_matrix(eng, fa, fb, H, sim):
    """pair_score over every (i, j) with ia = i, ib = n_a + j on the concatenated features"""
    na, nb = fa[0].shape[0], fb[0].shape[0]
    q, k, v = (torch.cat([a, b]).contiguous() for a, b in zip(fa, fb))
    ia = torch.arange(na, dtype=torch.int32).repeat_interleave(nb).cuda()
    ib = (na + torch.arange(nb, dtype=torch.int32)).repeat(na).cuda()
    return eng.pair_score(q, k, v, ia, ib, H, sim).view(na, nb)


TAP = dict(N=256, H=8, D=160)       # SD1.5's default tap: the persistent kernels


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("sim", ["cosine", "mse"])
@pytest.mark.parametrize("peaked", [False, True])
def test_default_tap_matrix_matches_float64_and_the_pair_path(eng, dtype, sim, peaked):
    """5 x 7 at the default tap; the peaked variant (logits of ~25 log2 units) moves the softmax reference point and rescales."""
    scale = 14.0 if peaked else 1.0
    fa = _feats(5, 21, dtype, **TAP, logit_scale=scale, correlate=0.6)
    fb = _feats(7, 22, dtype, **TAP, logit_scale=scale, correlate=0.6)
    got = eng.score_matrix(fa, fb, TAP["H"], sim)
    assert got.shape == (5, 7) and got.dtype == torch.float32
    want = _tail64(fa, fb, TAP["H"], sim, dtype)
    tol = 4e-3 if dtype == torch.bfloat16 else 5e-4
    if peaked:                  # (test_gpu_round6's peaked-logit tolerances of the pair tail)
        tol = 1e-2 if dtype == torch.bfloat16 else 2e-3
    g = got.double().cpu()
    if sim == "cosine":
        assert (g - want).abs().max().item() <= tol, (g, want)
    else:
        assert ((g - want).abs() / want.abs().clamp_min(1e-6)).max().item() <= 10 * tol, (g, want)
    # the self pass and the cross pass run the pair tail's step arithmetic and its products / fold: the same scores bit for bit
    assert torch.equal(got, _pair_matrix(eng, fa, fb, TAP["H"], sim))


@pytest.mark.parametrize("N,H,D,na,nb", [(256, 8, 160, 3, 4), (1024, 8, 80, 3, 4), (256, 16, 72, 3, 4), (1024, 20, 64, 2, 3),
                                         (4096, 8, 40, 2, 2)])
def test_fp32_matrix_matches_the_pair_path_and_float64(eng, N, H, D, na, nb):
    """The parity mode at the default tap and the generic shapes (SD1.5's other taps, DiT's 256 x 16 x 72, SDXL's 1024 x 20 x 64)."""
    fa = _feats(na, 31, torch.float32, N, H, D, correlate=0.5)
    fb = _feats(nb, 32, torch.float32, N, H, D, correlate=0.5)
    m = eng.score_matrix(fa, fb, H, "cosine")
    assert torch.equal(m, _pair_matrix(eng, fa, fb, H, "cosine"))      # pair_tail_kernel's attend, products and fold
    got = m.double().cpu()
    want = _tail64(fa, fb, H, "cosine", torch.float32)
    assert ((got - want).abs() / want.abs().clamp_min(1e-6)).max().item() <= 1e-5, (got, want)


@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float16, 256, 8, 160), (torch.float32, 256, 8, 160),
                                         (torch.bfloat16, 1024, 8, 80), (torch.float32, 256, 16, 72)])
def test_diagonal_and_symmetry(eng, dtype, N, H, D):
    """score_matrix(F, F): 1 on the diagonal (cosine), exactly 0 (mse) -- the self and cross passes run the same arithmetic on the
    same operands; score_matrix(F, G) == score_matrix(G, F).T bit for bit."""
    f = _feats(4, 41, dtype, N, H, D, correlate=0.4)
    g = _feats(3, 42, dtype, N, H, D, correlate=0.4)
    c = eng.score_matrix(f, f, H, "cosine")
    assert (c.diagonal() - 1.0).abs().max().item() <= 1e-6, c.diagonal()
    m = eng.score_matrix(f, f, H, "mse")
    assert torch.equal(m.diagonal(), torch.zeros(4, device=m.device)), m.diagonal()
    for sim in ("cosine", "mse"):
        assert torch.equal(eng.score_matrix(f, g, H, sim), eng.score_matrix(g, f, H, sim).T)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_determinism_and_slice_invariance(eng, dtype):
    """23 x 37 at the default tap (more units than one round of persistent workgroups): repeat calls, one row, and a column slice
    scored alone are bit-identical to the full matrix."""
    fa = _feats(23, 51, dtype, **TAP, correlate=0.4)
    fb = _feats(37, 52, dtype, **TAP, correlate=0.4)
    H = TAP["H"]
    for sim in ("cosine", "mse"):
        m1 = eng.score_matrix(fa, fb, H, sim)
        assert torch.equal(m1, eng.score_matrix(fa, fb, H, sim))
        row = eng.score_matrix(tuple(t[5:6].contiguous() for t in fa), fb, H, sim)
        assert torch.equal(row[0], m1[5])
        cols = eng.score_matrix(fa, tuple(t[11:20].contiguous() for t in fb), H, sim)
        assert torch.equal(cols, m1[:, 11:20])


@pytest.mark.parametrize("dtype,N,H,D", [(torch.float16, 256, 8, 160), (torch.bfloat16, 1024, 8, 80), (torch.float32, 256, 8, 160)])
def test_non_finite_gallery_features_flag_their_column(eng, dtype, N, H, D):
    fa = _feats(3, 61, dtype, N, H, D)
    fb = _feats(4, 62, dtype, N, H, D)
    fb[2][2, 1, 17, 100] = float("inf")
    s, st = eng.score_matrix(fa, fb, H, "cosine", return_status=True)
    want = torch.zeros(3, 4, dtype=torch.int32)
    want[:, 2] = 1
    assert torch.equal(st.cpu(), want)
    assert torch.isfinite(s[:, [0, 1, 3]]).all()


def test_invalid_arguments_raise(eng):
    from diffsim_amd import _lib
    fa = _feats(2, 71, torch.bfloat16, 256, 8, 160)
    fb = _feats(2, 72, torch.float16, 256, 8, 160)
    with pytest.raises(_lib.DsimError):
        eng.score_matrix(fa, fb, 8)
    L = _lib.lib()
    assert L.dsim_score_matrix_workspace_bytes(0, 3, 2, 8, 256, 160, _lib.DSIM_BF16) == 0
    need = L.dsim_score_matrix_workspace_bytes(2, 2, 2, 8, 256, 160, _lib.DSIM_BF16)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty(2, 2, device="cuda")
    q, k, v = fa
    rc = L.dsim_score_matrix(q.data_ptr(), k.data_ptr(), v.data_ptr(), 2, q.data_ptr(), k.data_ptr(), v.data_ptr(), 2, 2, 8, 256, 160,
                             _lib.DSIM_BF16, 0, out.data_ptr(), None, ws.data_ptr(), need // 2, None)
    assert rc != 0 and b"workspace" in L.dsim_strerror(rc).lower()
    rc = L.dsim_score_matrix(q.data_ptr(), k.data_ptr(), v.data_ptr(), 2, q.data_ptr(), k.data_ptr(), v.data_ptr(), 2, 2, 8, 256, 160,
                             7, 0, out.data_ptr(), None, ws.data_ptr(), need, None)
    assert rc != 0


# ---- end to end on the tiny graph ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_env():
    from diffsim_amd import config as C, synth as S
    from oracle import cpu_ref as R
    sd = S.make_state_dict(C.TINY, seed=0)
    return dict(sd=sd, oracle=R.build_unet(R.TINY, sd), ctx=S.make_context(C.TINY), R=R, C=C, S=S)


def _tiny_lats(env, n, off):
    zs = [env["S"].make_pair_latents(env["C"].TINY, off + i)[0] for i in range(n)]
    return torch.cat(zs)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_tiny_latent_matrix_equals_per_pair_scores(tiny_env, dtype):
    from diffsim_amd.diffsim import DiffSim
    C, S, ctx = tiny_env["C"], tiny_env["S"], tiny_env["ctx"]
    ds = DiffSim(torch_dtype=dtype, device="cuda", unet_config=C.TINY, state_dict=tiny_env["sd"])
    la, lb = _tiny_lats(tiny_env, 3, 0), _tiny_lats(tiny_env, 4, 10)
    n = S.draw_pair_noise(2334, la[:1].shape)
    for sim in ("cosine", "mse"):
        m = ds.score_latent_matrix(la, lb, n[2], n[3], ctx, "up_blocks", 0, 600, sim, batch=2).cpu()
        A = la.repeat_interleave(4, 0)
        Bm = lb.repeat(3, 1, 1, 1)
        p = ds.score_latent_pairs(A, Bm, n[2], n[3], ctx, "up_blocks", 0, 600, sim).view(3, 4).cpu()
        if dtype == torch.float32:
            assert ((m - p).abs() / p.abs().clamp_min(1e-6)).max().item() <= 1e-5, (m, p)
        else:
            assert ((m - p).abs() / p.abs().clamp_min(1e-3)).max().item() <= 4e-3, (m, p)
    if dtype == torch.float32:
        R, unet = tiny_env["R"], tiny_env["oracle"]
        m = ds.score_latent_matrix(la, lb, n[2], n[3], ctx, "up_blocks", 0, 600, "cosine").cpu()
        for i in range(3):
            for j in range(4):
                so = float(R.diffsim_latents(unet, la[i:i + 1], lb[j:j + 1], n[2], n[3], ctx, 600, "up_blocks", 0, "cosine"))
                assert abs(float(m[i, j]) - so) <= 1e-4 * max(abs(so), 1e-3), (i, j, float(m[i, j]), so)


# ---- end to end at SD1.5's full size: the default tap (up_blocks[0] at 512 px = 256 tokens x 8 heads x 160) ----------------------
def _oracle_unet(R, rcfg, sd, shapes):
    """Oracle U-Net without materialising random-init parameters first (meta construction + assign; the unused tail of the
    graph gets zero tensors)"""
    with torch.device("meta"):
        m = R.UNet2DConditionModel(rcfg)
    full = {k: (sd[k] if k in sd else torch.zeros(shp)) for k, shp in shapes.items()}
    m.load_state_dict(full, strict=True, assign=True)
    return m.eval()


def test_full_size_latent_matrix_fp32_against_the_oracle_and_bf16_against_pairs():
    """3 queries x 4 gallery latents at 512 px: fp32 cells within 1e-4 relative of the CPU oracle's per-pair score (oracle features
    + the float64 tail), bf16 cells -- the persistent sdpa160 self pass and matrix_cross160_kernel -- equal to score_latent_pairs."""
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim import DiffSim
    from oracle import cpu_ref as R
    cfg = C.SD15
    shapes = C.unet_param_shapes(cfg)
    sd = S.make_state_dict(cfg, seed=0, keys=[k for k in shapes if not k.startswith(("up_blocks.2", "up_blocks.3", "conv_norm_out", "conv_out"))])
    ctx = S.make_context(cfg)
    n = S.draw_pair_noise(2334, (1, 4, 64, 64))
    lat = [S.make_pair_latents(cfg, i) for i in range(4)]
    la = torch.cat([lat[0][0], lat[1][0], lat[2][0]])
    lb = torch.cat([lat[0][1], lat[1][1], lat[3][0], lat[3][1]])
    unet = _oracle_unet(R, R.SD15, sd, shapes)
    fa = [R.features(unet, la[i:i + 1], n[2], ctx) for i in range(3)]
    fb = [R.features(unet, lb[j:j + 1], n[3], ctx) for j in range(4)]
    want = torch.tensor([[float(R.pair_score(*fa[i], *fb[j])) for j in range(4)] for i in range(3)], dtype=torch.float64)
    del unet
    ds = DiffSim(torch_dtype=torch.float32, device="cuda", unet_config=cfg, state_dict=sd)
    got = ds.score_latent_matrix(la, lb, n[2], n[3], ctx, "up_blocks", 0, 600, "cosine").double().cpu()
    assert ((got - want).abs() / want.abs().clamp_min(1e-6)).max().item() <= 1e-4, (got, want)
    del ds
    torch.cuda.empty_cache()
    db = DiffSim(torch_dtype=torch.bfloat16, device="cuda", unet_config=cfg, state_dict=sd)
    assert db.engine("up_blocks", 0).heads == 8
    for sim in ("cosine", "mse"):
        m = db.score_latent_matrix(la, lb, n[2], n[3], ctx, "up_blocks", 0, 600, sim)
        p = db.score_latent_pairs(la.repeat_interleave(4, 0), lb.repeat(3, 1, 1, 1), n[2], n[3], ctx, "up_blocks", 0, 600, sim)
        assert torch.equal(m, p.view(3, 4)), (m, p)
    assert (db.score_latent_matrix(la, lb, n[2], n[3], ctx).double().cpu() - want).abs().max().item() <= 5e-3


# ---- image files through every scorer kind -------------------------------------------------------------------------------------
def _image_files(tmp_path, n, seed):
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    paths = []
    for i in range(n):
        base = torch.rand(3, 1, 1, generator=g) * 255
        px = (base + 60 * torch.randn(3, 160, 144, generator=g)).clamp(0, 255).to(torch.uint8)
        p = tmp_path / f"img{seed}_{i}.png"
        Image.fromarray(px.permute(1, 2, 0).numpy()).save(p)
        paths.append(str(p))
    return paths


def _assert_cells(m, want, rel=1e-5):
    want = torch.as_tensor(want, dtype=torch.float64)
    got = m.double().cpu()
    assert got.shape == want.shape
    assert ((got - want).abs() / want.abs().clamp_min(1e-6)).max().item() <= rel, (got, want)


def test_path_matrix_sd15_hip_vae_equals_score_pairs(tmp_path):
    """2 x 3 image files through the HIP VAE (decode, device preprocessing, one encode per chunk, slot-A / slot-B draws)
    against DiffSim.score_pairs on the same six pairs, both similarities."""
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.engine import VAEEncoder
    from diffsim_amd.retrieval import score_path_matrix
    ctx = S.make_context(C.TINY)
    vae = VAEEncoder(C.VAE_TINY, S.make_state_dict(C.VAE_TINY, seed=3), torch.float32)
    ds = DiffSim(torch_dtype=torch.float32, device="cuda", unet_config=C.TINY, state_dict=S.make_state_dict(C.TINY, seed=0),
                 vae=vae, encode_prompt=lambda p: ctx)
    qa, gb = _image_files(tmp_path, 2, 1), _image_files(tmp_path, 3, 2)
    pairs = [(a, b) for a in qa for b in gb]
    for sim in ("cosine", "mse"):
        m = score_path_matrix(ds, qa, gb, 128, "a cat", "up_blocks", 0, 600, 2334, sim)
        want = ds.score_pairs(pairs, 128, "a cat", "up_blocks", 0, 600, seed=2334, similarity=sim).view(2, 3)
        _assert_cells(m, want.cpu())
    m = ds.score_matrix(qa, gb, 128, "a cat", "up_blocks", [0], 600, seed=2334, similarity="cosine")
    _assert_cells(m, [[float(ds.diffsim(a, b, 128, "a cat", "up_blocks", [0], 600, seed=2334)) for b in gb] for a in qa])


def test_path_matrix_without_a_hip_vae_equals_per_pair_calls(tmp_path):
    """The scorer's own prepare_image_latents (no HIP VAE): the generator state behind slot A's draw starts every gallery draw.
    Against DiffSim.diffsim per pair, which reseeds and encodes both images."""
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.retrieval import score_path_matrix
    from tests._fakes import FakeVAE
    ctx = S.make_context(C.TINY)
    ds = DiffSim(torch_dtype=torch.float32, device="cuda", unet_config=C.TINY, state_dict=S.make_state_dict(C.TINY, seed=0),
                 vae=FakeVAE(), encode_prompt=lambda p: ctx)
    qa, gb = _image_files(tmp_path, 2, 3), _image_files(tmp_path, 3, 4)
    m = score_path_matrix(ds, qa, gb, 128, "a cat", "up_blocks", 1, 500, 2334, "cosine")
    _assert_cells(m, [[float(ds.diffsim(a, b, 128, "a cat", "up_blocks", 1, 500, seed=2334)) for b in gb] for a in qa])


def test_path_matrix_diffsim_xl(tmp_path):
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim_xl import diffsim_xl
    from diffsim_amd.retrieval import score_path_matrix
    from tests._fakes import FakeVAE
    ctx, pooled = S.make_context(C.SDXL_TINY), S.make_pooled(C.SDXL_TINY)
    xl = diffsim_xl(torch.float32, "cuda", unet_config=C.SDXL_TINY, state_dict=S.make_state_dict(C.SDXL_TINY, seed=0), vae=FakeVAE(),
                    encode_prompt=lambda p: (ctx, pooled))
    qa, gb = _image_files(tmp_path, 2, 5), _image_files(tmp_path, 3, 6)
    for sim in ("cosine", "mse"):
        m = score_path_matrix(xl, qa, gb, 128, "a cat", "up_blocks", [0, 1, 2], 600, 2334, sim)
        _assert_cells(m, [[float(xl.diffsim_score(a, b, 128, "a cat", "up_blocks", [0, 1, 2], 600, sim, 2334).reshape(-1)[0])
                           for b in gb] for a in qa])


def test_path_matrix_diffsim_dit(tmp_path):
    from diffsim_amd import config as C, synth as S
    from diffsim_amd.diffsim_dit import diffsim_DiT
    from diffsim_amd.retrieval import score_path_matrix
    from tests._fakes import FakeVAE
    dd = diffsim_DiT(128, 600, "cuda", dit_config=C.DIT_TINY, state_dict=S.make_state_dict(C.DIT_TINY, seed=0), vae=FakeVAE(),
                     torch_dtype=torch.float32)
    qa, gb = _image_files(tmp_path, 2, 7), _image_files(tmp_path, 3, 8)
    m = score_path_matrix(dd, qa, gb, 128, "p", "none", [2], 600, 2334, "cosine")
    _assert_cells(m, [[float(dd.diffsim_score(a, b, 128, "p", "none", [2], 600, "cosine", 2334).reshape(-1)[0]) for b in gb]
                      for a in qa])
