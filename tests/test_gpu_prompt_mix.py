"""Many prompts in one U-Net forward (a context table: dsim_unet_qkv_ctx / dsim_unet_qkv_taps_ctx, the engine's ctx_index, the
scorers' per-pair / per-triplet / per-image prompts): every row must be bit for bit what a one-prompt call gives that row."""
import ctypes as C_
import functools
import math

import pytest
import torch

from diffsim_amd import config as C, synth as S

pytestmark = pytest.mark.gpu

# per-image prompt assignments of 5 images: all equal, all distinct, uneven (5 images over 3 prompts)
ASSIGN = {"equal": [0, 0, 0, 0, 0], "distinct": [0, 1, 2, 3, 4], "uneven": [2, 0, 2, 1, 0]}
TAPS3 = [("down_blocks", 0), ("mid_blocks", 0), ("up_blocks", 1)]      # SD15_SMALL: d = 40 | 40, 80, 160 | ... 160, 80 on the way


@functools.lru_cache(maxsize=None)
def _sd(cfg):
    return S.make_state_dict(cfg, seed=0)


@functools.lru_cache(maxsize=None)
def _ds(cfg, dtype, dedup=True, graphs=False):
    from diffsim_amd.diffsim import DiffSim
    return DiffSim(torch_dtype=dtype, device="cuda", unet_config=cfg, state_dict=_sd(cfg), dedup_cfg=dedup, use_graphs=graphs)


def _ctxs(cfg, k):
    return [S.make_context(cfg, seed=100 + i) for i in range(k)]


def _images(cfg, n):
    lat = [S.make_pair_latents(cfg, i) for i in range((n + 1) // 2)]
    z = torch.cat([t for p in lat for t in p])[:n]
    nz = S.draw_pair_noise(2334, z[:1].shape)
    return z, torch.cat([nz[2 + i % 2] for i in range(n)])


def _pairs(cfg, n):
    lat = [S.make_pair_latents(cfg, i) for i in range(n)]
    nz = S.draw_pair_noise(2334, lat[0][0].shape)
    return torch.cat([p[0] for p in lat]), torch.cat([p[1] for p in lat]), nz[2], nz[3]


def _rows_equal(got, want, rows, what):
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, what
        assert torch.equal(g[rows], w[rows]), what


@pytest.mark.parametrize("assign", sorted(ASSIGN))
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cfg", ["SD15_SMALL", "TINY"])
def test_features_per_image_prompts(cfg, dtype, assign):
    """SD15_SMALL reaches the 16-bit short-key cross-attention at d = 40 / 80 / 160, TINY at d = 64 and the exact kernel at
    d = 16 / 32; every row of a mixed call equals the row of a one-prompt call over the same images."""
    cfg = getattr(C, cfg)
    ds = _ds(cfg, dtype)
    lat, nz = _images(cfg, 5)
    ctxs = _ctxs(cfg, 5)
    idx = ASSIGN[assign]
    prompts = [ctxs[i] for i in idx]
    taps = TAPS3 if cfg is C.SD15_SMALL else [("down_blocks", 1), ("mid_blocks", 0), ("up_blocks", 2)]
    for b, l in taps:
        got = ds.features(lat, nz, prompts, b, l, 600)
        for p in sorted(set(idx)):
            rows = torch.tensor([i for i, j in enumerate(idx) if j == p])
            _rows_equal(got, ds.features(lat, nz, ctxs[p], b, l, 600), rows, (b, l, p))


@pytest.mark.parametrize("dedup", [True, False])
@pytest.mark.parametrize("cfg,dtype", [("TINY", torch.float32), ("TINY", torch.bfloat16), ("SD15_SMALL", torch.float16)])
def test_features_taps_per_image_prompts(cfg, dtype, dedup):
    """A tap sweep with mixed prompts, CFG de-duplication on and off."""
    from diffsim_amd.sweep import all_taps
    cfg = getattr(C, cfg)
    ds = _ds(cfg, dtype, dedup)
    lat, nz = _images(cfg, 5)
    ctxs = _ctxs(cfg, 3)
    idx = ASSIGN["uneven"]
    # (a tap in the first down block turns de-duplication off: leave it out where de-duplication is under test)
    taps = [t for t in all_taps(cfg) if t != ("down_blocks", 0)] if dedup else all_taps(cfg)
    got = ds.features_taps(lat, nz, [ctxs[i] for i in idx], taps, 600)
    for p in sorted(set(idx)):
        rows = torch.tensor([i for i, j in enumerate(idx) if j == p])
        want = ds.features_taps(lat, nz, ctxs[p], taps, 600)
        for t, tap in enumerate(taps):
            _rows_equal(got[t], want[t], rows, (tap, p))


def _per_prompt_scores(ds, la, lb, nA, nB, prompts, **kw):
    """Pair i's one-prompt score: one call per distinct prompt over every pair, row i taken from its prompt's call."""
    out = torch.empty(la.shape[0], dtype=torch.float32, device="cuda")
    for p in {id(p): p for p in prompts}.values():
        s = ds.score_latent_pairs(la, lb, nA, nB, p, **kw)
        for i, q in enumerate(prompts):
            if q is p:
                out[i] = s[i]
    return out


def test_score_latent_pairs_streams_and_graphs():
    """Per-pair prompts over several chunks on two streams; and hipGraph replays of one shape with two different prompt
    assignments, each equal to the eager result (a replay must not keep the assignment of its capture)."""
    cfg = C.TINY
    la, lb, nA, nB = _pairs(cfg, 7)
    ctxs = _ctxs(cfg, 3)
    first = [ctxs[i] for i in (0, 1, 2, 1, 0, 2, 2)]
    second = [ctxs[i] for i in (2, 2, 0, 1, 1, 0, 1)]
    eager = _ds(cfg, torch.bfloat16)
    for prompts in (first, second):
        want = _per_prompt_scores(eager, la, lb, nA, nB, prompts, batch_pairs=7, streams=1)
        assert torch.equal(eager.score_latent_pairs(la, lb, nA, nB, prompts, batch_pairs=2, streams=2), want)
        assert torch.equal(eager.score_latent_pairs(la, lb, nA, nB, prompts, batch_pairs=7, streams=1), want)
    graphs = _ds(cfg, torch.bfloat16, graphs=True)
    for prompts in (first, second, first):
        want = eager.score_latent_pairs(la, lb, nA, nB, prompts, batch_pairs=4, streams=1)
        assert torch.equal(graphs.score_latent_pairs(la, lb, nA, nB, prompts, batch_pairs=4), want)
    assert any(k[-1] == 3 for k in graphs._base._graphs)          # (the mixed chunks did run as replays of a captured graph)


def test_sd15_full_size_32_distinct_prompts():
    """64 x 64 latents, bf16: 32 pairs with 32 distinct contexts in one forward against one call per pair."""
    cfg = C.SD15
    ds = _ds(cfg, torch.bfloat16)
    la, lb, nA, nB = _pairs(cfg, 32)
    ctxs = _ctxs(cfg, 32)
    got = ds.score_latent_pairs(la, lb, nA, nB, ctxs, batch_pairs=32)
    want = torch.stack([ds.score_latent_pairs(la[i:i + 1], lb[i:i + 1], nA, nB, ctxs[i])[0] for i in range(32)])
    assert torch.equal(got, want)


def test_one_prompt_path_launches_unchanged():
    """A per-image list that names one prompt runs exactly the one-prompt launches; a table adds one gather and projects every
    batch element's context."""
    cfg = C.TINY
    ds = _ds(cfg, torch.bfloat16)
    eng = ds.engine("up_blocks", 0)
    lat, nz = _images(cfg, 4)
    ctxs = _ctxs(cfg, 2)

    def recs(prompt):
        eng.profile(True)
        ds.features(lat, nz, prompt, "up_blocks", 0, 600)
        r = [(fam, shape) for fam, _fl, _by, _ms, shape in eng.profile_records(detail=True)]
        eng.profile(False)
        return r
    one = recs(ctxs[0])
    assert recs([ctxs[0]] * 4) == one
    mixed = recs([ctxs[0], ctxs[1], ctxs[1], ctxs[0]])
    assert [f for f, _ in mixed if f.startswith("ctx_gather")] == ["ctx_gather_bf16"]
    assert len(mixed) == len(one) + 1
    L, Dc = cfg.ctx_len, cfg.cross_attention_dim
    kv = lambda r, m: [s for _f, s in r if s.startswith(f"M{m} ") and s.endswith(f" K{Dc}")]      # the K / V projections
    assert kv(one, 2 * L) and len(kv(mixed, 8 * L)) == len(kv(one, 2 * L)) and not kv(mixed, 2 * L)


def test_profiled_engine_destroyed_with_records_pending():
    """A handle destroyed while it still holds the records of a profiled forward (HIP events included) releases them with its
    weights: closing is safe to repeat, and the next handle's features and records are its own."""
    from diffsim_amd.diffsim import DiffSim
    cfg = C.TINY
    lat, nz = _images(cfg, 2)
    ctx = _ctxs(cfg, 1)[0]
    want = _ds(cfg, torch.bfloat16).features(lat, nz, ctx, "up_blocks", 0, 600)
    counts = []
    for _ in range(2):
        ds = DiffSim(torch_dtype=torch.bfloat16, device="cuda", unet_config=cfg, state_dict=_sd(cfg))
        eng = ds.engine("up_blocks", 0)
        eng.profile(True)
        got = ds.features(lat, nz, ctx, "up_blocks", 0, 600)
        counts.append(len(eng.profile_records()))
        eng.close()                         # records pending: never cleared by profile(False)
        assert not eng._h.value
        eng.close()
        for g, w in zip(got, want):
            assert torch.equal(g, w)
    assert counts[0] > 0 and counts[0] == counts[1]


def _image_files(root, n, seed):
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    paths = []
    for i in range(n):
        base = torch.rand(3, 1, 1, generator=g) * 255
        px = (base + 60 * torch.randn(3, 80, 72, generator=g)).clamp(0, 255).to(torch.uint8)
        p = root / f"img{seed}_{i}.png"
        Image.fromarray(px.permute(1, 2, 0).numpy()).save(p)
        paths.append(str(p))
    return paths


def test_harness_nights_csv_one_forward_per_chunk(tmp_path):
    """A NIGHTS-shaped csv with 3 prompts: the rank shard runs as one group (ceil(n / unet_triplets) forwards, not one or more
    per prompt), each prompt encoded once, every score bit for bit the per-triplet diffsim call's."""
    import csv
    from diffsim_amd import harness as H
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.engine import VAEEncoder
    from diffsim_amd.sweep import score_path_triplets_taps
    cfg = C.TINY
    words = ["cat", "dog", "tree"]
    table = {f"An image of a {w}": S.make_context(cfg, seed=200 + i) for i, w in enumerate(words)}
    encoded = []

    def encode(p):
        encoded.append(p)
        return table[p]
    vae = VAEEncoder(C.VAE_TINY, S.make_state_dict(C.VAE_TINY, seed=3), torch.float32)
    ds = DiffSim(torch_dtype=torch.bfloat16, device="cuda", unet_config=cfg, state_dict=_sd(cfg), vae=vae, encode_prompt=encode)
    im = _image_files(tmp_path, 6, 5)
    order = [0, 1, 2, 0, 0, 2, 1]
    with open(tmp_path / "data.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["split", "ref_path", "left_path", "right_path", "left_vote", "prompt"])
        for j, o in enumerate(order):
            w.writerow(["val", im[j % 6], im[(j + 1) % 6], im[(j + 3) % 6], j % 2, words[o].upper()])
    rows = H.read_nights_csv(str(tmp_path))
    trip = [(r["ref"], r["left"], r["right"], r["prompt"]) for r in rows]
    n, ut = len(trip), 4          # (grouped by prompt, the 7 triplets would take 3 forwards: cat 3, dog 2, tree 2)
    ds.engine("up_blocks", 1)
    base = ds._base
    calls = {"qkv": 0, "qkv_taps": 0}
    for name in calls:
        fn = getattr(base, name)

        def spy(*a, _fn=fn, _name=name, **kw):
            calls[_name] += 1
            return _fn(*a, **kw)
        setattr(base, name, spy)
    s_ab, s_ac, bad = H.score_path_triplets(ds, trip, 128, "up_blocks", 1, 600, 2334, "cosine", batch_triplets=4, unet_triplets=ut)
    assert bad == 0 and calls["qkv"] == math.ceil(n / ut)
    assert sorted(encoded) == sorted(table)
    taps = [("up_blocks", 1), ("mid_blocks", 0)]
    ds._ctx.clear()
    encoded.clear()
    t_ab, t_ac = score_path_triplets_taps(ds, trip, 128, taps, 600, 2334, "cosine", batch_triplets=4, unet_triplets=ut)
    assert calls["qkv_taps"] == math.ceil(n / ut)
    assert sorted(encoded) == sorted(table)
    assert torch.equal(t_ab[0], s_ab) and torch.equal(t_ac[0], s_ac)
    for j, (a, b, c, p) in enumerate(trip):
        assert torch.equal(s_ab[j:j + 1], ds.diffsim(a, b, 128, p, "up_blocks", 1, 600, seed=2334)), j
        assert torch.equal(s_ac[j:j + 1], ds.diffsim(a, c, 128, p, "up_blocks", 1, 600, seed=2334)), j
        assert torch.equal(t_ab[1, j:j + 1], ds.diffsim(a, b, 128, p, "mid_blocks", 0, 600, seed=2334)), j


def test_sdxl_refuses_a_context_table():
    """SDXL's pooled prompt embedding enters the per-half time embedding: n_ctx > 1 is refused by the C ABI (before any launch)
    and by the engine; an SD1.5 handle refuses a table without an index and n_ctx < 1."""
    from diffsim_amd import _lib
    from diffsim_amd.diffsim_xl import diffsim_xl
    from diffsim_amd.engine import _stream_ptr
    cfg = C.SDXL_TINY
    xl = diffsim_xl(torch.bfloat16, "cuda", unet_config=cfg, state_dict=S.make_state_dict(cfg, seed=0))
    ctx, pooled = S.make_context(cfg), S.make_pooled(cfg)
    lat, nz = _images(cfg, 2)
    xl.features(lat, nz, ctx, pooled, "up_blocks", [0, 0, 0], 600)         # the handle is conditioned, ready to run
    eng = xl.engine("up_blocks", [0, 0, 0])
    L = _lib.lib()
    h = eng._h
    table = torch.stack([ctx, S.make_context(cfg, seed=5)]).cuda()
    idx = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    lat_d, nz_d = lat.cuda(), nz.cuda()
    shape = (2, 2, eng.tokens, eng.heads * eng.head_dim)
    q, k, v = (torch.empty(shape, dtype=torch.bfloat16, device="cuda") for _ in range(3))
    wsb = eng.workspace_bytes(2)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    assert L.dsim_unet_ctx_workspace_bytes(h, 2, 2) == 0 and L.dsim_unet_ctx_workspace_bytes(h, 2, 1) == wsb
    st = L.dsim_unet_qkv_ctx(h, lat_d.data_ptr(), nz_d.data_ptr(), 0.5, 0.5, table.data_ptr(), 2, idx.data_ptr(), 2, q.data_ptr(),
                             k.data_ptr(), v.data_ptr(), ws.data_ptr(), wsb, _stream_ptr())
    assert st == -1
    tap = (_lib.TapC * 1)()
    tap[0].block, tap[0].layer, tap[0].attn, tap[0].tfm = 2, 0, 0, 0
    ptr = lambda t: (C_.c_void_p * 1)(t.data_ptr())
    st = L.dsim_unet_qkv_taps_ctx(h, lat_d.data_ptr(), nz_d.data_ptr(), 0.5, 0.5, table.data_ptr(), 2, idx.data_ptr(), 2, 1, tap,
                                  ptr(q), ptr(k), ptr(v), ws.data_ptr(), wsb, _stream_ptr())
    assert st == -1
    torch.cuda.synchronize()
    with pytest.raises(_lib.DsimError):
        eng.qkv(lat_d, nz_d, 0.5, 0.5, table, ctx_index=[0, 1])
    from diffsim_amd.harness import score_latent_triplets
    with pytest.raises(ValueError):         # two prompts for two triplets: SDXL batches take one
        score_latent_triplets(xl, lat, lat, lat, nz[:1], nz[1:], [(ctx, pooled), (table[1].cpu(), pooled)])
    # SD1.5 handle: the argument checks of the new entry points
    sd = _ds(C.TINY, torch.bfloat16)
    e = sd.engine("up_blocks", 0)
    la, nzz = _images(C.TINY, 2)
    sd.features(la, nzz, S.make_context(C.TINY), "up_blocks", 0, 600)
    tb = torch.stack(_ctxs(C.TINY, 2)).cuda()
    la_d, nz2 = la.cuda(), nzz.cuda()
    shape = (2, 2, e.tokens, e.heads * e.head_dim)
    q, k, v = (torch.empty(shape, dtype=torch.bfloat16, device="cuda") for _ in range(3))
    wsb = e.workspace_bytes(2, 2)
    assert wsb > e.workspace_bytes(2) > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    args = lambda n_ctx, ip: (e._h, la_d.data_ptr(), nz2.data_ptr(), 0.5, 0.5, tb.data_ptr(), n_ctx, ip, 2, q.data_ptr(), k.data_ptr(),
                              v.data_ptr(), ws.data_ptr(), wsb, _stream_ptr())
    assert L.dsim_unet_qkv_ctx(*args(2, None)) == -1
    assert L.dsim_unet_qkv_ctx(*args(0, idx.data_ptr())) == -1
    torch.cuda.synchronize()
