"""The device resize's host half: the numpy restatement of PIL's 8-bit resampling against PIL itself (this test DEFINES the served
range: every size here lies inside ``resize.served`` and must give PIL's bytes), the int32 accumulator's range, the range
predicate, the decode-only request of the decode pool, and the wiring (CLI flag, C ABI symbols).  No GPU."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from diffsim_amd import resize as rz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_FILTER = {"lanczos": Image.Resampling.LANCZOS, "bicubic": Image.Resampling.BICUBIC}
EXTENTS = (16, 17, 23, 31, 64, 100, 257, 1000)


def image(w, h, seed=0):
    """Random bytes with saturated blocks and stripes, so that the filters' overshoot clips at 0 and at 255."""
    a = np.random.default_rng(seed + 7919 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    a[: max(1, h // 3), : max(1, w // 2)] = 255
    a[h // 2:, w // 3: w // 2 + 1] = 0
    a[:, 2 * w // 3:: 7] = 255
    a[3 * h // 4:: 5, : w // 4] = 0
    return a


def pil_resize(a, out_w, out_h, filt, crop=None):
    im = Image.fromarray(a).resize((out_w, out_h), resample=PIL_FILTER[filt])
    if crop is not None:
        ox, oy, cw, ch = crop
        im = im.crop((ox, oy, ox + cw, oy + ch))
    return np.asarray(im)


def outputs(w, h):
    """The issue's three outputs for a (w, h) source: (out_w, out_h, crop)."""
    ow, oh = rz.shortest_edge(w, h, 56)
    return [(64, 64, None), (96, 64, None), (ow, oh, ((ow - 48) // 2, (oh - 48) // 2, 48, 48))]


@pytest.mark.parametrize("filt", ["lanczos", "bicubic"])
def test_restatement_is_pil_bit_for_bit(filt):
    cases = [(w, h, o) for w in EXTENTS for h in EXTENTS for o in outputs(w, h)]
    cases += [(768, 768, (512, 512, None)), (2048, 1536, (512, 512, None))]
    # tall sources up to the range's aspect bound (h = 64 w), where PIL still runs the horizontal pass first
    cases += [(w, h, o) for w, h in ((16, 1024), (20, 1280), (100, 6400)) for o in ((64, 512, None), (224, 224, None), (96, 128, None))]
    bad = []
    for w, h, (ow, oh, crop) in cases:
        assert rz.served(w, h, ow, oh), (w, h, ow, oh)              # the test defines the served range: nothing in it is skipped
        a = image(w, h)
        diff = int((rz.resize_reference(a, ow, oh, filt, crop) != pil_resize(a, ow, oh, filt, crop)).sum())
        if diff:
            bad.append((w, h, ow, oh, crop, diff))
    assert not bad, bad


def test_accumulators_stay_inside_int32():
    sizes = {(s, o) for s in EXTENTS for o in (64, 96, 56)} | {(s, int(56 * s / t)) for s in EXTENTS for t in EXTENTS if t <= s}
    sizes |= {(768, 512), (2048, 512), (1536, 512), (16384, 256), (4032, 512), (3024, 224)}
    worst = 0
    for filt in rz.FILTERS:
        for s, o in sorted(sizes):
            if s == o:
                continue
            bounds, kk = rz.coeff_table(s, o, filt)
            assert bounds.dtype == np.int32 and kk.dtype == np.int32 and bounds.shape == (o, 2) and kk.shape[0] == o
            assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(1) <= s).all()
            assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()      # what the kernels' tiles rely on
            assert (bounds[:, 1] <= kk.shape[1]).all()
            reach = int(np.abs(kk.astype(np.int64)).sum(1).max()) * 255 + (1 << 21)
            assert reach < (1 << 31), (filt, s, o, reach)
            worst = max(worst, reach)
    print(f"largest |acc| bound: {worst / (1 << 31):.3f} * 2^31")


def test_coeff_table_is_cached_and_read_only():
    b, k = rz.coeff_table(100, 64, "lanczos")
    assert rz.coeff_table(100, 64, "lanczos")[0] is b
    with pytest.raises(ValueError):
        k[0, 0] = 1
    assert rz.filter_name(Image.Resampling.BICUBIC) == "bicubic" and rz.filter_name(Image.Resampling.LANCZOS) == "lanczos"
    assert rz.filter_name(Image.Resampling.BILINEAR) is None and rz.filter_name("nearest") is None


def test_served_range():
    assert rz.served(768, 768, 512, 512) and rz.served(16, 16, 64, 64) and rz.served(4096, 16, 64, 64)
    assert not rz.served(8, 1000, 224, 224) and not rz.served(2, 300, 64, 64) and not rz.served(5, 300, 64, 64)
    assert not rz.served(4097, 100, 64, 64) and rz.served(4096, 100, 64, 64)            # more than 64 source pixels per output pixel
    assert not rz.served(100, 6500, 64, 100)
    assert not rz.served(16385, 16385, 512, 512) and not rz.served(100, 100, 0, 10)
    # at most 64 widths tall: beyond 100 widths PIL's bytes are vertical-first (the test below); wide sources have no such bound
    assert rz.served(16, 1000, 64, 64) and rz.served(16, 1024, 64, 64) and not rz.served(16, 1025, 64, 64)
    assert not rz.served(16, 1900, 64, 64) and not rz.served(24, 3000, 224, 224) and not rz.served(128, 16384, 256, 256)
    assert not rz.served(100, 12500, 224, 224) and rz.served(100, 6400, 224, 224) and rz.served(1900, 16, 64, 64)


def test_tall_sources_are_why_the_range_stops_at_64_widths():
    """Recorded, not relied on: with both passes and h > 100 w, PIL's bytes are not the horizontal-first restatement's.  Everything
    the device path serves stays below 64 widths; sizes between 64 and 100 widths fall back although they would match."""
    for w, h, o in ((8, 1000, 224), (16, 1640, 64), (16, 1900, 224)):
        a = image(w, h)
        assert not rz.served(w, h, o, o)
        print(f"{w}x{h} -> {o}x{o} differing bytes:", int((rz.resize_reference(a, o, o, "lanczos") != pil_resize(a, o, o, "lanczos")).sum()))
    for w, h in ((12, 1000), (16, 1600)):               # below 100 widths: horizontal-first
        a = image(w, h)
        assert np.array_equal(rz.resize_reference(a, 224, 224, "lanczos"), pil_resize(a, 224, 224, "lanczos"))
    a = image(16, 1900)                                  # one pass skipped: no corner
    assert np.array_equal(rz.resize_reference(a, 16, 64, "lanczos"), pil_resize(a, 16, 64, "lanczos"))


@pytest.mark.parametrize("procs", [0, 2])
def test_decode_pool_raw_round_trip(procs, tmp_path):
    from diffsim_amd.image import DecodePool
    paths, arrays = [], []
    for i, (w, h) in enumerate([(100, 80), (33, 47), (64, 64)]):
        a = image(w, h, i)
        p = str(tmp_path / f"im{i}.png")
        Image.fromarray(a).save(p)
        paths.append(p)
        arrays.append(a)
    pool = DecodePool(procs)
    try:
        raw = [f.result() for f in pool.submit_raw(paths + [Image.fromarray(arrays[1])])]
        assert [r.shape for r in raw] == [(80, 100, 3), (47, 33, 3), (64, 64, 3), (47, 33, 3)]
        assert all(r.dtype == np.uint8 and np.array_equal(r, a) for r, a in zip(raw, arrays + [arrays[1]]))
        old = DecodePool.gather(pool.submit(paths, 32)).numpy()                      # the old request, on the same workers
        assert np.array_equal(old, np.stack([pil_resize(a, 32, 32, "lanczos") for a in arrays]))
        with pytest.raises(Exception):
            pool.submit_raw([str(tmp_path / "missing.png")])[0].result()
        assert np.array_equal(pool.submit_raw(paths[:1])[0].result(), arrays[0])    # a failed request leaves the worker usable
    finally:
        pool.shutdown()


def test_worker_answers_the_old_request_with_the_old_bytes(tmp_path):
    a = image(50, 40)
    p = str(tmp_path / "a.png")
    Image.fromarray(a).save(p)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", "from diffsim_amd._decode_worker import serve; serve()"],
                       input=f"24\t{p}\nraw\t{p}\n".encode(), capture_output=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    px = pil_resize(a, 24, 24, "lanczos").tobytes()
    assert r.stdout[:8 + len(px)] == struct.pack("<q", len(px)) + px                # <length><pixels>, nothing else
    rest = r.stdout[8 + len(px):]
    assert rest == struct.pack("<qii", a.nbytes + 8, 40, 50) + a.tobytes()


def test_wiring():
    from diffsim_amd import _lib, cli
    from diffsim_amd.scorer import Scorer
    assert cli.arg_parse(["--gpu_resize"]).gpu_resize is True and cli.arg_parse([]).gpu_resize is False
    assert Scorer.gpu_resize is False
    hdr = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    L = _lib.lib()
    for name in ("dsim_resize_u8_workspace_bytes", "dsim_resize_u8"):
        assert name in _lib.SYMBOLS and hasattr(L, name) and re.search(rf"\b{name}\(", hdr), name
    assert re.search(r"#define\s+DSIM_ABI_VERSION\s+7\b", hdr) and _lib.ABI_VERSION == 7            # additive: the version stays
    assert "resize.hip" in __import__("diffsim_amd.build", fromlist=["SOURCES"]).SOURCES
    # the refusals need no device: a workspace query of 0
    import ctypes as C
    img = (_lib.ResizeImageC * 1)()
    img[0].w, img[0].h, img[0].h_table, img[0].v_table, img[0].rows = 64, 64, -1, -1, 64
    tab = (_lib.ResizeTableC * 1)()
    tab[0].in_size, tab[0].out_size, tab[0].ksize = 1, 1, 1
    q = L.dsim_resize_u8_workspace_bytes
    assert q(img, 1, tab, 1, 4, 64, 64, 0, 0, 64, 64, 3 * 64 * 64) > 0
    assert q(img, 0, tab, 1, 4, 64, 64, 0, 0, 64, 64, 3 * 64 * 64) == 0
    assert q(img, 1, tab, 1, 4, 64, 64, 1, 0, 64, 64, 3 * 64 * 64) == 0             # the crop leaves the image
    assert q(img, 1, tab, 1, 4, 64, 64, 0, 0, 64, 64, 3 * 64 * 64 - 1) == 0         # the image leaves the buffer
    assert q(C.cast(None, C.POINTER(_lib.ResizeImageC)), 1, tab, 1, 4, 64, 64, 0, 0, 64, 64, 3 * 64 * 64) == 0
