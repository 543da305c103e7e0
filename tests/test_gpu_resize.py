"""The device resize (csrc/resize.hip, engine.resize_u8) against PIL, bit for bit (``torch.equal`` everywhere: PIL's 8-bit
resampling is integer arithmetic, so there is no tolerance), the independence of a batch's images, the host fallback, the
refusals of the C ABI, and the files-in paths with ``gpu_resize`` on against off.  Shapes: sources of a few hundred pixels with a
64 x 64 / 96 x 64 / crop-48 output -- widths that are no multiple of the 64-column tile or of 4 bytes, more row blocks than one,
both skipped passes, an upscale, and a 1024-wide source for long tap rows."""
import ctypes as C_
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from diffsim_amd import _lib, config as C, resize as rz, synth as S
from tests.test_resize_host import image, pil_resize

SOURCES = [(97, 64), (64, 97), (200, 150), (33, 300), (512, 40), (40, 48), (129, 129), (64, 64), (1024, 640)]      # (w, h)


@pytest.fixture(scope="module")
def sources():
    return [image(w, h, i) for i, (w, h) in enumerate(SOURCES)]


def _want(arrays, ow, oh, filt, crop=None):
    return torch.from_numpy(np.stack([pil_resize(a, ow, oh, filt, crop) for a in arrays]))


# ---- 1. the kernels against PIL --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ow,oh,filt", [(64, 64, "lanczos"), (96, 64, "bicubic")])
def test_ragged_batch_is_pil(ow, oh, filt, sources):
    from diffsim_amd.engine import RESIZE_COUNTS, resize_u8
    before = dict(RESIZE_COUNTS)
    got = resize_u8(sources, ow, oh, filt)
    assert got.shape == (len(sources), oh, ow, 3) and got.dtype == torch.uint8 and got.is_cuda
    want = _want(sources, ow, oh, filt)
    for i, wh in enumerate(SOURCES):
        assert torch.equal(got[i].cpu(), want[i]), (wh, int((got[i].cpu() != want[i]).sum()))
    assert RESIZE_COUNTS["gpu"] - before["gpu"] == len(sources) and RESIZE_COUNTS["fallback"] == before["fallback"]


@pytest.mark.parametrize("filt", ["bicubic", "lanczos"])
def test_shortest_edge_and_centre_crop_is_pil(filt):
    from diffsim_amd.engine import resize_u8
    for w, h in ((200, 150), (150, 200)):
        a = image(w, h, 3)
        ow, oh = rz.shortest_edge(w, h, 56)
        crop = ((ow - 48) // 2, (oh - 48) // 2, 48, 48)
        got = resize_u8([a, a[::-1].copy()], ow, oh, filt, crop)
        assert got.shape == (2, 48, 48, 3)
        assert torch.equal(got.cpu(), _want([a, a[::-1].copy()], ow, oh, filt, crop)), (w, h)
    # a window that is no multiple of anything, off centre, on both passes and on each skipped pass
    for (w, h), (ow, oh) in (((200, 150), (75, 56)), ((75, 150), (75, 56)), ((200, 56), (75, 56)), ((75, 56), (75, 56))):
        a = image(w, h, 4)
        crop = (5, 3, 61, 47)
        assert torch.equal(resize_u8([a], ow, oh, filt, crop).cpu(), _want([a], ow, oh, filt, crop)), (w, h, ow, oh)


# ---- 2. an image's bytes are its own ---------------------------------------------------------------------------------------------
def test_batch_independence(sources):
    from diffsim_amd.engine import resize_u8
    full = resize_u8(sources, 64, 64, "lanczos")
    assert torch.equal(resize_u8(sources, 64, 64, "lanczos"), full)                 # two calls, equal bits
    for i, a in enumerate(sources):
        assert torch.equal(resize_u8([a], 64, 64, "lanczos")[0], full[i]), SOURCES[i]
    perm = [4, 8, 0, 7, 2, 6, 1, 3, 5]
    assert torch.equal(resize_u8([sources[i] for i in perm], 64, 64, "lanczos"), full[perm])
    assert torch.equal(resize_u8([torch.from_numpy(a) for a in sources[:3]], 64, 64, "lanczos"), full[:3])       # host tensors


def test_chunked_uploads_give_the_same_bytes(sources, monkeypatch):
    from diffsim_amd import engine
    full = engine.resize_u8(sources, 64, 64, "lanczos")
    monkeypatch.setattr(engine, "RESIZE_CHUNK_BYTES", 100_000)                     # several chunks; the 1024 x 640 source alone
    assert torch.equal(engine.resize_u8(sources, 64, 64, "lanczos"), full)


# ---- 3. the fallback -------------------------------------------------------------------------------------------------------------
def test_fallback_outside_the_served_range():
    from diffsim_amd.engine import RESIZE_COUNTS, resize_u8
    a, b, c = image(5, 300), image(16, 16), image(40, 30)
    d, e = image(16, 1900), image(16, 1024)                     # more than 64 widths tall: PIL's pass order differs there; at the bound
    assert not rz.served(5, 300, 64, 64) and rz.served(16, 16, 64, 64) and not rz.served(16, 1900, 64, 64) and rz.served(16, 1024, 64, 64)
    before = dict(RESIZE_COUNTS)
    got = resize_u8([a, b, c, d, e], 64, 64, "lanczos")
    assert RESIZE_COUNTS["fallback"] - before["fallback"] == 2 and RESIZE_COUNTS["gpu"] - before["gpu"] == 3
    assert torch.equal(got.cpu(), _want([a, b, c, d, e], 64, 64, "lanczos"))
    with pytest.raises(_lib.DsimError):
        resize_u8([a], 64, 64, "bilinear")
    with pytest.raises(_lib.DsimError):
        resize_u8([b], 64, 64, "lanczos", (10, 0, 60, 64))
    with pytest.raises(_lib.DsimError):
        resize_u8([b[:, :, :2]], 64, 64, "lanczos")


# ---- 4. the C ABI's refusals -----------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing():
    L = _lib.lib()
    w, h, ow, oh = 100, 80, 64, 64
    a = image(w, h)
    hb, hk = rz.coeff_table(w, ow, "lanczos")
    vb, vk = rz.coeff_table(h, oh, "lanczos")
    ints = np.concatenate([hb.reshape(-1), hk.reshape(-1), vb.reshape(-1), vk.reshape(-1)]).astype(np.int32)
    tables_dev = torch.from_numpy(ints).cuda()
    src = torch.from_numpy(a.reshape(-1).copy()).cuda()
    out = torch.full((1, oh, ow, 3), 7, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def args(**kw):
        img = (_lib.ResizeImageC * 1)()
        img[0].src_offset, img[0].w, img[0].h, img[0].h_table, img[0].v_table = kw.get("src_offset", 0), kw.get("w", w), kw.get("h", h), \
            kw.get("h_table", 0), kw.get("v_table", 1)
        img[0].y_first, img[0].rows, img[0].temp_offset = 0, h, 0
        tab = (_lib.ResizeTableC * 2)()
        tab[0].offset, tab[0].in_size, tab[0].out_size, tab[0].ksize = 0, kw.get("w", w), ow, kw.get("ksize", hk.shape[1])
        tab[1].offset, tab[1].in_size, tab[1].out_size, tab[1].ksize = hb.size + hk.size, kw.get("h", h), oh, vk.shape[1]
        geo = (kw.get("ow", ow), kw.get("oh", oh), kw.get("ox", 0), kw.get("oy", 0), kw.get("cw", ow), kw.get("ch", oh))
        return img, tab, geo, kw.get("n", 1), kw.get("n_tables", 2), kw.get("src_bytes", src.numel())

    def call(ws, ws_bytes, null=None, **kw):
        img, tab, geo, n, nt, sb = args(**kw)
        ptr = {"src": src.data_ptr(), "tables": tables_dev.data_ptr(), "out": out.data_ptr(), "ws": ws.data_ptr(), "img": img, "tab": tab}
        if null in ("img", "tab"):
            ptr[null] = C_.cast(None, C_.POINTER(_lib.ResizeImageC if null == "img" else _lib.ResizeTableC))
        elif null:
            ptr[null] = None
        q = L.dsim_resize_u8_workspace_bytes(ptr["img"], n, ptr["tab"], nt, ints.size, *geo, sb)
        rc = L.dsim_resize_u8(ptr["src"], sb, ptr["img"], n, ptr["tables"], ints.size, ptr["tab"], nt, *geo, ptr["out"], ptr["ws"],
                              ws_bytes, stream)
        return q, rc

    img, tab, geo, n, nt, sb = args()
    need = L.dsim_resize_u8_workspace_bytes(img, n, tab, nt, ints.size, *geo, sb)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    invalid = [dict(n=0), dict(ow=0), dict(oh=0), dict(cw=0), dict(ch=0), dict(ox=1), dict(oy=60, ch=5), dict(w=0), dict(h=0),
               dict(ksize=0), dict(src_bytes=3 * w * h - 1), dict(src_offset=16), dict(h_table=2), dict(v_table=2), dict(n_tables=1)]
    for kw in invalid:
        q, rc = call(ws, need, **kw)
        assert (q, rc) == (0, -1), kw
    for null in ("img", "tab"):
        assert call(ws, need, null=null) == (0, -1), null
    for null in ("src", "tables", "out", "ws"):                 # the query takes none of these: the call refuses
        assert call(ws, need, null=null)[1] == -1, null
    q, rc = call(ws, need - 1)
    assert q == need and rc == -3
    torch.cuda.synchronize()
    assert bool((out == 7).all())                               # nothing was enqueued
    assert call(ws, need) == (need, 0)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _want([a], ow, oh, "lanczos"))


# ---- 5. files in: the switch on against off -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("resize_files")
    paths = []
    for i, (w, h) in enumerate([(100, 80), (64, 64), (80, 100), (97, 131)]):
        p = str(d / f"im{i}.png")
        Image.fromarray(image(w, h, 10 + i)).save(p)
        paths.append(p)
    return paths


def _same(x, y):
    return torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y


def _diffsim(dtype=torch.float32):
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.engine import VAEEncoder
    ctx = S.make_context(C.TINY)
    return DiffSim(torch_dtype=dtype, device="cuda", unet_config=C.TINY, state_dict=S.make_state_dict(C.TINY, seed=0),
                   vae=VAEEncoder(C.VAE_TINY, S.make_state_dict(C.VAE_TINY, seed=3), torch.float32), encode_prompt=lambda p: ctx)


def test_path_latents_and_diffsim_with_the_switch(files):
    from diffsim_amd.inputs import path_latents
    ds = _diffsim()
    rows = [(files[0], files[1]), (files[2], files[3]), (files[1], files[0])]
    assert ds.gpu_resize is False
    off = path_latents(ds, rows, (0, 1), 64, 2333, 2)
    s_off = ds.diffsim(files[0], files[1], 64, "p", "up_blocks", [0], 600, seed=2334)
    p_off = ds.score_pairs(rows, 64, "p", "up_blocks", [0], 600)
    ds.gpu_resize = True
    on = path_latents(ds, rows, (0, 1), 64, 2333, 2)
    for x, y in zip(off[0] + list(off[1:]), on[0] + list(on[1:])):
        assert torch.equal(x, y)
    assert _same(ds.diffsim(files[0], files[1], 64, "p", "up_blocks", [0], 600, seed=2334), s_off)
    assert _same(ds.diffsim(Image.open(files[0]), Image.open(files[1]), 64, "p", "up_blocks", [0], 600, seed=2334), s_off)
    assert torch.equal(ds.score_pairs(rows, 64, "p", "up_blocks", [0], 600), p_off)


def test_preprocess_batch_is_preprocess_call(files):
    from diffsim_amd.vit import CLIP_MEAN, CLIP_STD, Preprocess
    arrays = [np.asarray(Image.open(p).convert("RGB")) for p in files] + [image(5, 300), image(300, 47)]
    for resample in (Image.Resampling.BICUBIC, Image.Resampling.LANCZOS, Image.Resampling.BILINEAR):
        pre = Preprocess(48, 40, CLIP_MEAN, CLIP_STD, resample)
        want = torch.cat([pre(Image.fromarray(a)) for a in arrays])
        got = pre.batch(arrays, torch.device("cuda:0"))
        assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got.cpu(), want), resample


@pytest.mark.parametrize("kind", ["clip", "dinov2"])
def test_vit_cross_scores_with_the_switch(kind, files):
    from diffsim_amd import harness as H
    from diffsim_amd.vit import CLIPScore, Dinov2Score, Preprocess, CLIP_MEAN, CLIP_STD, IMAGENET_MEAN, IMAGENET_STD
    cfg = C.VIT_TINY_CLIP if kind == "clip" else C.VIT_TINY_DINO
    pre = Preprocess(48, 40, *((CLIP_MEAN, CLIP_STD) if kind == "clip" else (IMAGENET_MEAN, IMAGENET_STD)))
    sc = (CLIPScore if kind == "clip" else Dinov2Score)(cfg, S.make_state_dict(cfg, 3), "cuda", torch.float32, pre)
    cross = sc.clip_cross_score if kind == "clip" else sc.dino_cross_score
    a, b, c, d = files
    trip = [(a, b, c, "p"), (d, c, a, "q"), (b, a, d, "p")]
    off = (cross([a, c], [b, d], [1]), cross(Image.open(a), Image.open(b), [2]),
           H.score_path_triplets(sc, trip, 512, "up_blocks", [1], 600, 2333, "cosine", batch_triplets=2, unet_triplets=2))
    sc.gpu_resize = True
    on = (cross([a, c], [b, d], [1]), cross(Image.open(a), Image.open(b), [2]),
          H.score_path_triplets(sc, trip, 512, "up_blocks", [1], 600, 2333, "cosine", batch_triplets=2, unet_triplets=2))
    assert torch.equal(off[0], on[0]) and torch.equal(off[1], on[1])
    assert torch.equal(off[2][0], on[2][0]) and torch.equal(off[2][1], on[2][1]) and off[2][2] == on[2][2] == 0


# ---- 6. the command line --------------------------------------------------------------------------------------------------------
def test_cli_gpu_resize_prints_the_same_accuracy(tmp_path, capsys, files):
    from diffsim_amd import cli
    from diffsim_amd.engine import RESIZE_COUNTS
    from tests.test_vit_host import _write_checkpoint
    ckpt, tree = str(tmp_path / "ckpt"), str(tmp_path / "cute")
    _write_checkpoint(ckpt, C.VIT_TINY_DINO)
    n = 0
    for cls in ("mug", "shoe"):
        for inst in ("inst0", "inst1"):
            folder = os.path.join(tree, cls, inst, "light0")
            os.makedirs(folder)
            for j in range(2):
                Image.open(files[n % 4]).rotate(90 * (n // 4), expand=True).save(os.path.join(folder, f"im{j}.png"))
                n += 1
    base = ["--metric", "dino_cross", "--dataset", "cute", "--model_path", ckpt, "--image_path", tree, "--target_layer", "1",
            "--similarity", "cosine", "--dtype", "fp32", "--decode_procs", "0"]
    assert cli.main(base) == 0
    plain = capsys.readouterr().out
    before = dict(RESIZE_COUNTS)
    assert cli.main(base + ["--gpu_resize"]) == 0
    text = capsys.readouterr().out
    pick = lambda t: [ln for ln in t.splitlines() if ln.startswith(("Total", "Accuracy", "2x Accuracy"))]
    assert pick(plain) and pick(plain) == pick(text), (plain, text)
    assert "GPU resize:" not in plain
    done = RESIZE_COUNTS["gpu"] - before["gpu"]
    assert f"GPU resize: {RESIZE_COUNTS['gpu']} image(s) resized on the device, {RESIZE_COUNTS['fallback']} fell back to the host" in text
    assert done == 120, done                                    # 40 triplets, three images each
