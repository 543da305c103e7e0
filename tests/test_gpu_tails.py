"""The tiled score tails -- pair_tail_kernel (engine.pair_score), pair_map_kernel (engine.pair_score_maps) and matrix_tail_kernel
(engine.score_matrix), one pair_tail_body / attend / tail_products between them -- against the float64 tail of tests/_tail64.py at
every tap they serve: SD1.5's and SDXL's levels, DiT-XL/2's, the ragged token counts of odd image sides (side 28: 784 / 196 / 49,
side 26: 169 / 49, ...), the 4096-token levels and every head dim of DSIM_FOR_EACH_D, in bf16, fp16 and fp32.  The 16-bit default
tap (256 x 8 x 160) belongs to the persistent attn160 kernels and is tested with them.

Gates are test_gpu_maps' (the pair tail's): fp32 1e-5 relative, 16-bit cosine _score_tol absolute, mse 10 x that relative,
LOCAL_GATE for the 16-bit per-token maps.  DSIM_TAILS_LOG=<file> appends each case's largest errors there."""
import math
import os

import pytest
import torch

from tests._tail64 import Tail64
from tests.test_gpu_maps import LOCAL_GATE, _local_err, _score_err, _score_tol

pytestmark = pytest.mark.gpu

B = 2
ALL = (torch.bfloat16, torch.float16, torch.float32)
TAILS_LOG = os.environ.get("DSIM_TAILS_LOG")


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


def _feats(n, seed, dtype, N, H, D, logit_scale=1.0, correlate=0.5):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(n, B, N, H * D, generator=g) for _ in range(3))
    base = tuple(torch.randn(1, B, N, H * D, generator=g) for _ in range(3))
    q, k, v = (correlate * b + (1 - correlate) * t for b, t in zip(base, (q, k, v)))
    q = q * logit_scale
    return tuple(t.to(dtype).cuda().contiguous() for t in (q, k, v))


def _idx(*xs):
    return torch.tensor(list(xs), dtype=torch.int32).cuda()


SHAPES = [(4096, 8, 40), (1024, 8, 80), (64, 8, 160),                           # SD1.5 512 px: 64 x 64, 32 x 32, the mid block
          (4096, 10, 64), (1024, 20, 64),                                       # SDXL 1024 px
          (256, 16, 72),                                                        # DiT-XL/2
          (784, 8, 40), (196, 8, 80), (49, 8, 160), (16, 8, 160),               # SD1.5 at side 28 (224 px) and 16 tokens
          (169, 10, 64), (49, 20, 64)]                                          # SDXL at side 26
EDGES = [(N, 4, d) for N in (1, 31, 127, 129) for d in (16, 32, 40)]
CASES = ([(dt, N, H, D, False) for dt in ALL for N, H, D in SHAPES + EDGES] +
         [(torch.float32, 256, 8, 160, False)] +                                # (16-bit goes to attn160 there)
         [(dt, 4095, 4, d, False) for dt, d in zip(ALL, (40, 16, 32))] +        # one past a 64-key tile short of 4096
         [(dt, N, H, D, True) for dt in ALL for N, H, D in ((784, 8, 40), (4096, 8, 40))])


def _case_id(c):
    dt, N, H, D, peaked = c
    return f"{str(dt)[6:]}-N{N}-H{H}-D{D}" + ("-peaked" if peaked else "")


def _log(dtype, sim, N, H, D, peaked, **errs):
    if TAILS_LOG:
        with open(TAILS_LOG, "a") as f:
            f.write(f"{str(dtype)[6:]} {sim} N={N} H={H} D={D} peaked={peaked} " +
                    " ".join(f"{k}={v:.3e}" for k, v in errs.items()) + "\n")


@pytest.mark.parametrize("dtype,N,H,D,peaked", CASES, ids=[_case_id(c) for c in CASES])
def test_tails_match_float64_and_each_other(eng, dtype, N, H, D, peaked):
    """pair_score, pair_score_maps and score_matrix on one feature set: scores, local and contrib against float64; the matrix equal
    to pair_score over its cells bit for bit; the maps' score equal to the pair path's within 1e-6 and to 0.5 * sum(contrib)."""
    big = N >= 4095
    n, na = (3, 1) if big else (5, 2)              # the matrix: images [0, na) against [na, n)
    q, k, v = _feats(n, 1000 * H + 7 * N + D, dtype, N, H, D, logit_scale=14.0 if peaked else 1.0)
    pairs = [(0, 1), (2, 0)] if big else [(0, 2), (1, 4), (3, 0)]       # (the last: B's image first, its directions swapped)
    ia, ib = _idx(*(a for a, _ in pairs)), _idx(*(b for _, b in pairs))
    fa = tuple(t[:na].contiguous() for t in (q, k, v))
    fb = tuple(t[na:].contiguous() for t in (q, k, v))
    ca = torch.arange(na, dtype=torch.int32).repeat_interleave(n - na).cuda()
    cb = (na + torch.arange(n - na, dtype=torch.int32)).repeat(na).cuda()
    ref = Tail64(q, k, v, H, dtype)
    tol = _score_tol(dtype, peaked)
    for sim in ("cosine", "mse"):
        gate = tol if sim == "cosine" else 10 * tol
        ps = eng.pair_score(q, k, v, ia, ib, H, sim)
        ms, ml, mc = eng.pair_score_maps(q, k, v, ia, ib, H, sim)
        mat = eng.score_matrix(fa, fb, H, sim)
        assert mat.shape == (na, n - na) and ml.shape == (len(pairs), 2, N) and mc.shape == ml.shape
        # the matrix's self pass and cross pass are the pair tail's attend, rounding, products and fold: bit-identical cells
        assert torch.equal(mat.flatten(), eng.pair_score(q, k, v, ca, cb, H, sim)), (mat, sim)
        e_score = e_local = e_contrib = 0.0
        for p, (a, b) in enumerate(pairs):
            ws, wl, wc = ref.pair(a, b, sim)
            for got in (float(ps[p]), float(ms[p])):
                e = _score_err(got, ws, sim, dtype)
                e_score = max(e_score, e)
                assert e <= gate, (sim, p, got, ws)
            gl, gc = ml[p].double().cpu(), mc[p].double().cpu()
            # N * contrib is a token's share of the score at the scale of local (for mse it is local)
            if dtype == torch.float32:
                el, ec = (gl - wl).abs().max().item(), (N * (gc - wc)).abs().max().item()
                assert el <= 1e-5 and ec <= 1e-5, (sim, p, el, ec)
            else:
                el, ec = _local_err(gl, wl, sim), _local_err(N * gc, N * wc, sim)
                assert el <= LOCAL_GATE[(dtype, sim)] and ec <= LOCAL_GATE[(dtype, sim)], (sim, p, el, ec)
            e_local, e_contrib = max(e_local, el), max(e_contrib, ec)
            gs = float(ms[p])
            assert abs(0.5 * mc[p].double().sum().item() - gs) <= 1e-6 * max(1.0, abs(gs)), (sim, p)
            assert abs(gs - float(ps[p])) <= 1e-6 * max(1.0, abs(float(ps[p]))), (sim, p, gs, float(ps[p]))
        for i in range(na):
            for j in range(n - na):
                ws = ref.pair(i, na + j, sim)[0]
                e = _score_err(float(mat[i, j]), ws, sim, dtype)
                e_score = max(e_score, e)
                assert e <= gate, (sim, i, j, float(mat[i, j]), ws)
        _log(dtype, sim, N, H, D, peaked, score=e_score, local=e_local, contrib=e_contrib)


RAGGED = [(1, 4, 16), (31, 4, 32), (49, 8, 160), (127, 4, 40), (129, 4, 16), (169, 10, 64), (196, 8, 80), (784, 8, 40)]


@pytest.mark.parametrize("N,H,D", RAGGED)
@pytest.mark.parametrize("dtype", ALL)
def test_ragged_tail_properties(eng, dtype, N, H, D):
    """At token counts that are no multiple of the 128-query tile: the matrix diagonal (an image against itself) is 1 / exactly 0;
    a pair scored alone equals the same pair inside a batch; swapping a pair's roles keeps its score and swaps its maps' directions;
    SimilarityMaps puts a square N on its s x s grid."""
    from diffsim_amd.maps import SimilarityMaps
    f = _feats(4, 77 + N + D, dtype, N, H, D, correlate=0.4)
    c = eng.score_matrix(f, f, H, "cosine")
    assert (c.diagonal() - 1.0).abs().max().item() <= 1e-6, c.diagonal()
    m = eng.score_matrix(f, f, H, "mse")
    assert torch.equal(m.diagonal(), torch.zeros(4, device=m.device)), m.diagonal()
    q, k, v = f
    ia, ib = _idx(0, 1, 3, 2, 1), _idx(2, 3, 0, 2, 0)
    for sim in ("cosine", "mse"):
        s = eng.pair_score(q, k, v, ia, ib, H, sim)
        mp = eng.pair_score_maps(q, k, v, ia, ib, H, sim)
        for p in range(ia.numel()):
            one_a, one_b = ia[p:p + 1].clone(), ib[p:p + 1].clone()
            assert torch.equal(eng.pair_score(q, k, v, one_a, one_b, H, sim)[0], s[p]), (sim, p)
            assert all(torch.equal(x[0], y[p]) for x, y in zip(eng.pair_score_maps(q, k, v, one_a, one_b, H, sim), mp)), (sim, p)
        assert torch.equal(eng.pair_score(q, k, v, ib, ia, H, sim), s)
        sw = eng.pair_score_maps(q, k, v, ib, ia, H, sim)
        assert torch.equal(sw[0], mp[0]) and torch.equal(sw[1], mp[1].flip(1)) and torch.equal(sw[2], mp[2].flip(1))
        side = math.isqrt(N)
        if side * side == N:
            sm = SimilarityMaps(*mp)
            assert sm.grid == (side, side) and sm.local.shape == (5, 2, side, side)
            assert torch.equal(sm.local[1, 0, (N - 1) // side, (N - 1) % side], mp[1][1, 0, N - 1])
        else:
            with pytest.raises(ValueError):
                SimilarityMaps(*mp)


# ---- engine.pair_score's argument checks: each refusal is raised before any launch -------------------------------------------
def _bad_args(kind):
    q, k, v = _feats(3, 5, torch.bfloat16, 64, 4, 32)
    ia, ib, H = _idx(0, 1), _idx(1, 2), 4
    if kind == "q_not_4d":
        q = q.reshape(3 * B, 64, 128)
    elif kind == "k_fewer_images":
        k = k[:2].contiguous()
    elif kind == "v_other_tokens":
        v = v[:, :, :32].contiguous()
    elif kind == "q_not_contiguous":
        q = torch.cat([q, q], dim=3)[..., :128]
    elif kind == "idx_not_contiguous":
        ib = _idx(1, 0, 2, 0)[::2]
    elif kind == "heads_do_not_divide":
        H = 3
    elif kind == "idx_lengths_differ":
        ib = _idx(1)
    return q, k, v, ia, ib, H


@pytest.mark.parametrize("kind", ["q_not_4d", "k_fewer_images", "v_other_tokens", "q_not_contiguous", "idx_not_contiguous",
                                  "heads_do_not_divide", "idx_lengths_differ"])
def test_pair_score_refuses(eng, kind):
    from diffsim_amd import _lib
    args = _bad_args(kind)
    for status in (False, True):
        with pytest.raises(_lib.DsimError):
            eng.pair_score(*args, "cosine", return_status=status)


def test_pair_score_accepts_the_unmodified_arguments(eng):
    q, k, v, ia, ib, H = _bad_args(None)
    s = eng.pair_score(q, k, v, ia, ib, H, "cosine")
    assert s.shape == (2,) and torch.isfinite(s).all()
    assert (s - eng.pair_score_maps(q, k, v, ia, ib, H, "cosine")[0]).abs().max().item() <= 1e-6
