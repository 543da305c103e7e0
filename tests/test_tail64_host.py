"""The float64 tail reference of the GPU tail tests (tests/_tail64.py) checked on its own: chunked SDPA against torch's, the
reference's golden tail scores (tests/golden/g4_tail.npz), the maps summing to the score, and an image against itself."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests._tail64 import Tail64, heads64, matrix64, pairs64, sdpa64


def _feats(n, seed, N, H, D, dtype=torch.float32, Bc=2):
    g = torch.Generator().manual_seed(seed)
    base = tuple(torch.randn(1, Bc, N, H * D, generator=g) for _ in range(3))
    return tuple((0.5 * b + 0.5 * torch.randn(n, Bc, N, H * D, generator=g)).to(dtype) for b in base)


@pytest.mark.parametrize("N", [1, 49, 130])
@pytest.mark.parametrize("chunk", [None, 1, 16, 64])
def test_chunked_sdpa_equals_torch_sdpa(N, chunk):
    g = torch.Generator().manual_seed(N)
    q, k, v = (torch.randn(2, 3, N, 40, generator=g, dtype=torch.float64) * s for s in (3.0, 1.0, 1.0))
    want = F.scaled_dot_product_attention(q, k, v)
    got = sdpa64(q, k, v, chunk)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert (got - want).abs().max().item() <= 1e-12


def test_query_chunks_are_bounded_at_4096_tokens(monkeypatch):
    """A 4096-token call holds one chunk of scores at a time: the matmul producing scores never sees more than SCORE_BUDGET."""
    from tests import _tail64
    seen = []
    mm = torch.matmul

    def spy(a, b):
        out = mm(a, b)
        seen.append(out.numel())
        return out
    monkeypatch.setattr(_tail64.torch, "matmul", spy)
    q = torch.randn(2, 2, 4096, 16, dtype=torch.float64)
    sdpa64(q, q, q)
    assert max(seen) <= _tail64.SCORE_BUDGET and len(seen) > 2


def _f32_reduction_error(sa, sb, sim):
    """How far the reference's float32 cosine / mse of its own float32 SDPA outputs lies from the float64 products of the same
    outputs: the golden carries this error (at 2 x 8 x 256 x 160 the float32 cosine of 655,360 elements is off by ~1.3e-5
    relative), a float64 tail does not"""
    outs = [F.scaled_dot_product_attention(*x[:1], *y[1:]) for x, y in ((sa, sb), (sa, sa), (sb, sa), (sb, sb))]
    o32, o64 = outs, [o.double() for o in outs]

    def score(o):
        if sim == "cosine":
            return 0.5 * sum(float(F.cosine_similarity(x.reshape(1, -1), y.reshape(1, -1))) for x, y in ((o[0], o[1]), (o[2], o[3])))
        return 0.5 * (float(F.mse_loss(o[0], o[1])) + float(F.mse_loss(o[2], o[3])))
    return abs(score(o32) - score(o64))


def test_reproduces_the_golden_tail(golden_dir):
    """tests/golden/g4_tail.npz: every score, both similarities, under test_g4_score_tail's bounds (rtol 1e-6, atol 1e-7) plus
    the float32 reduction error the golden itself carries, measured on the spot."""
    g4 = np.load(os.path.join(golden_dir, "g4_tail.npz"))
    for i in range(10):
        shp = tuple(int(x) for x in g4[f"shape_{i}"])
        gen = torch.Generator("cpu").manual_seed(int(g4[f"seed_{i}"][0]))
        sets = [[torch.randn(shp, generator=gen) * (1.5 if j == 0 else 1.0) for j in range(3)] for _ in range(2)]
        mixw = 0.3 + 0.07 * i
        sets[1] = [mixw * a + (1 - mixw) * b for a, b in zip(sets[0], sets[1])]
        if i == 8:
            sets[1] = [t.clone() for t in sets[0]]
        Bc, H, N, D = shp
        q, k, v = (torch.stack([s[j].transpose(1, 2).reshape(Bc, N, H * D) for s in sets]) for j in range(3))
        for sim in ("cosine", "mse"):
            (score, _, _), = pairs64(q, k, v, [0], [1], H, sim, torch.float32)
            want = float(g4[f"score_{i}_{sim}"][0])
            e32 = _f32_reduction_error(sets[0], sets[1], sim)
            assert e32 <= 2e-5 * abs(want) + 1e-7, (i, sim, e32)
            assert abs(score - want) <= 1e-6 * abs(want) + 1e-7 + e32, (i, sim, score, want, e32)
            m = matrix64((q[:1], k[:1], v[:1]), (q[1:], k[1:], v[1:]), H, sim, torch.float32)
            assert m.shape == (1, 1) and float(m[0, 0]) == score


@pytest.mark.parametrize("N,H,D", [(1, 2, 16), (49, 4, 40), (130, 2, 32)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("sim", ["cosine", "mse"])
def test_maps_sum_to_the_score(N, H, D, dtype, sim):
    q, k, v = _feats(3, 7 + N, N, H, D, dtype)
    out = pairs64(q, k, v, [0, 2], [1, 0], H, sim, dtype, chunk=16)
    for score, local, contrib in out:
        assert local.shape == (2, N) and contrib.shape == (2, N) and local.dtype == torch.float64
        assert abs(0.5 * float(contrib.sum()) - score) <= 1e-12 * max(1.0, abs(score))
        if sim == "mse":            # a token's contrib is its local over N
            assert (contrib * N - local).abs().max().item() <= 1e-12 * max(1.0, local.abs().max().item())
    # swapping the roles swaps the directions
    sw = pairs64(q, k, v, [1], [0], H, sim, dtype)[0]
    assert sw[0] == pytest.approx(out[0][0], rel=1e-14, abs=1e-15)
    assert torch.allclose(sw[1], out[0][1].flip(0), rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_an_image_against_itself(dtype):
    q, k, v = _feats(2, 3, 49, 4, 40, dtype)
    for a in (0, 1):
        s, lo, co = pairs64(q, k, v, [a], [a], 4, "cosine", dtype)[0]
        assert abs(s - 1.0) <= 1e-12 and (lo - 1).abs().max().item() <= 1e-12
        s, lo, co = pairs64(q, k, v, [a], [a], 4, "mse", dtype)[0]
        assert s == 0.0 and not lo.any() and not co.any()
    m = matrix64((q, k, v), (q, k, v), 4, "mse", dtype)
    assert not m.diagonal().any() and (m - m.T).abs().max().item() <= 1e-15


def test_outputs_are_rounded_to_the_pipeline_dtype():
    q, k, v = _feats(2, 5, 31, 2, 16, torch.bfloat16)
    t = Tail64(q, k, v, 2, torch.bfloat16)
    o = t.attn(0, 1)
    assert torch.equal(o, o.to(torch.bfloat16).double())
    exact = sdpa64(heads64(q[0], 2), heads64(k[1], 2), heads64(v[1], 2))
    assert 0 < (o - exact).abs().max().item() <= 2 ** -8 * exact.abs().max().item()
