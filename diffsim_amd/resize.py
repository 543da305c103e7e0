"""PIL's 8-bit resampling restated: the coefficient tables the device resize reads, the range it serves, and a numpy reference.

``Image.resize`` on an RGB image (Pillow's Resample.c) is integer arithmetic over a fixed-point table: per output position a
window ``[xmin, xmin + n)`` of the source and n weights, built in double (``precompute_coeffs``), turned to 22-bit fixed point with
``int(+-0.5 + k * 2**22)`` (``normalize_coeffs_8bpc``), and applied as ``clip8((2**21 + sum(p * k)) >> 22)``: a horizontal pass over
the source rows the vertical table reads, into uint8, then a vertical pass.  An axis whose extent does not change is skipped.
``coeff_table`` builds the tables with Python floats and ``math.sin`` (the same doubles, the same libm), so the device kernels
(csrc/resize.hip, engine.resize_u8) and ``resize_reference`` give PIL's bytes; tests/test_resize_host.py holds both to that.
"""
from __future__ import annotations

import functools
import math
from typing import Optional, Tuple

import numpy as np

PRECISION_BITS = 32 - 8 - 2             # Resample.c: 8 bits of pixel, 2 of headroom for the filters' overshoot
MIN_SIDE, MAX_SIDE, MAX_RATIO, MAX_ASPECT = 16, 16384, 64, 64


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {"lanczos": (_lanczos, 3.0), "bicubic": (_bicubic, 2.0)}


def filter_name(resample) -> Optional[str]:
    """"lanczos" / "bicubic" for a filter name or the PIL resampling value of one, None for every other filter."""
    if isinstance(resample, str):
        return resample if resample in FILTERS else None
    return {1: "lanczos", 3: "bicubic"}.get(int(resample))


@functools.lru_cache(maxsize=512)
def coeff_table(in_size: int, out_size: int, filter: str) -> Tuple[np.ndarray, np.ndarray]:
    """(bounds int32 [out_size][2] = (xmin, n), coefficients int32 [out_size][ksize]) of one axis: precompute_coeffs over the whole
    axis (box = 0 .. in_size) followed by normalize_coeffs_8bpc.  Coefficients past n are 0.  The arrays are shared: read only."""
    fn, support = FILTERS[filter]
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"coeff_table: extents {in_size} -> {out_size}")
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            kk[xx, x] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)
        bounds[xx] = (xmin, xmax)
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return bounds, kk


def served(w: int, h: int, out_w: int, out_h: int) -> bool:
    """Whether the device path takes a (w, h) source to (out_w, out_h): both source sides in [16, 16384], at most 64 source pixels
    per output pixel on each axis, and a height of at most 64 widths.  The last bound is the one PIL's bytes need: when both passes
    run and h > 100 w (2 x 300, 8 x 1000, 16 x 1640, 50 x 5125: observed, the rule's source not found) PIL's result is that of the
    vertical pass run first, which this horizontal-first arithmetic does not give; 64 leaves a margin below the observed 100.  Wide,
    short sources and single-pass resizes show no such corner.  Everything outside goes through PIL on the host."""
    if out_w < 1 or out_h < 1:
        return False
    if not (MIN_SIDE <= w <= MAX_SIDE and MIN_SIDE <= h <= MAX_SIDE):
        return False
    if h > MAX_ASPECT * w:
        return False
    return w <= MAX_RATIO * out_w and h <= MAX_RATIO * out_h


def shortest_edge(w: int, h: int, resize: int) -> Tuple[int, int]:
    """(out_w, out_h) of the HF image processors' shortest-edge rule: the short side to `resize`, the long one to
    int(resize * long / short)."""
    short, long = (w, h) if w <= h else (h, w)
    ns, nl = int(resize), int(resize * long / short)
    return (ns, nl) if w <= h else (nl, ns)


def _pass(src: np.ndarray, bounds: np.ndarray, kk: np.ndarray, first: int, count: int) -> np.ndarray:
    """One pass along axis 0 of src [extent][...] u8 for output positions [first, first + count)."""
    out = np.empty((count,) + src.shape[1:], np.uint8)
    s = src.astype(np.int64)
    for j in range(count):
        xmin, n = int(bounds[first + j, 0]), int(bounds[first + j, 1])
        acc = np.tensordot(kk[first + j, :n].astype(np.int64), s[xmin:xmin + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        out[j] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_reference(array: np.ndarray, out_w: int, out_h: int, filter: str, crop=None) -> np.ndarray:
    """``Image.fromarray(array).resize((out_w, out_h), filter)`` for a uint8 (h, w, 3) array, then ``.crop`` to the window
    crop = (ox, oy, cw, ch) (None: the whole image), in numpy integers: the arithmetic the device kernels run."""
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("resize_reference: a uint8 (h, w, 3) array")
    h, w, _ = a.shape
    ox, oy, cw, ch = (0, 0, out_w, out_h) if crop is None else crop
    if cw < 1 or ch < 1 or ox < 0 or oy < 0 or ox + cw > out_w or oy + ch > out_h:
        raise ValueError(f"resize_reference: crop {crop} outside {out_w}x{out_h}")
    y0, rows = oy, ch
    if h != out_h:
        vb, vk = coeff_table(h, out_h, filter)
        y0 = int(vb[oy, 0])
        rows = int(vb[oy + ch - 1, 0] + vb[oy + ch - 1, 1]) - y0
    a = a[y0:y0 + rows]
    if w != out_w:
        hb, hk = coeff_table(w, out_w, filter)
        a = _pass(a.transpose(1, 0, 2), hb, hk, ox, cw).transpose(1, 0, 2)
    else:
        a = a[:, ox:ox + cw]
    if h != out_h:
        vb = vb.copy()
        vb[:, 0] -= y0
        a = _pass(a, vb, vk, oy, ch)
    return np.ascontiguousarray(a)
