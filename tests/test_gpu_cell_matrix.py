"""Cell-region score matrices (csrc/cell_matrix.hip behind dsim_score_matrix_cell_regions / _cell_weights;
engine.score_matrix_cell_regions / _cell_weights): the region and the soft score matrix with set B's rows belonging to the cell,
mask_b (n_a, n_b, N).  A cell is the region (soft region) score of its pair under (mask_a[i], mask_b[i][j]), so it is checked to the
bit against engine.pair_score_regions / pair_score_weights called per cell on that cell's two images and two rows, against the
region / soft matrix where the rows are equal along i, against engine.score_matrix where every row is full, against the float64
restatements tests/_region64.py and tests/_soft64.py under tests/test_gpu_region_matrix.py's gate, and for what the header promises.

n_a = 2 queries and n_b = 3 gallery images (non-square: a transposed cell index shows); tests/test_gpu_region_matrix.py's features.

Largest errors against float64 of the first MI355X run (test_unequal_cell_regions_match_float64; recorded, not used): see FIRST_RUN."""
import ctypes

import pytest
import torch

from tests._region64 import regions64
from tests._soft64 import soft64
from tests.test_gpu_region_matrix import _feats, _gate, _score_err

pytestmark = pytest.mark.gpu

B = 2
N_A, N_B = 2, 3
SHAPES = [(256, 2, 160), (144, 2, 72), (256, 4, 40), (64, 4, 32)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CASES = [(N, H, D, dt) for N, H, D in SHAPES for dt in DTYPES]
IDS = [f"{N}-{H}-{D}-{str(dt)[6:]}" for N, H, D, dt in CASES]
# first MI355X run at (256, 4, 40), largest error over the six cells, (regions, weights) per dtype and similarity; the gates are
# 1e-5 | 4e-3 | 5e-4 (cosine) and ten times that (mse)
FIRST_RUN = {("float32", "cosine"): (3.4e-08, 4.8e-08), ("float32", "mse"): (5.5e-08, 6.9e-08),
             ("bfloat16", "cosine"): (1.1e-06, 1.9e-05), ("bfloat16", "mse"): (1.2e-04, 1.3e-04),
             ("float16", "cosine"): (1.5e-06, 1.2e-06), ("float16", "mse"): (1.3e-05, 2.2e-05)}


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


def _cell_sizes(N, off=0):
    """[n_a][n_b] set-B row sizes drawn from {1, 63, 65, 128, 129, N - 1, N} (those that fit N), the two cells of a column always
    different; off = 0 and off = 3 together hold every size of the set"""
    cand = sorted({s for s in (1, 63, 65, 128, 129, N - 1, N) if 1 <= s <= N})
    return [[cand[(j + 2 * i + off) % len(cand)] for j in range(N_B)] for i in range(N_A)]


def _rows(N, sizes, seed, weights=False):
    """(len(sizes), N) rows on the GPU with sizes[r] tokens on at seeded (scattered) positions: bool masks, or uint8 weights with the
    on tokens' bytes uniform in 1 .. 255"""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(len(sizes), N, dtype=torch.uint8 if weights else torch.bool)
    for r, s in enumerate(sizes):
        pos = torch.randperm(N, generator=g)[:s]
        m[r, pos] = torch.randint(1, 256, (s,), generator=g).to(torch.uint8) if weights else True
    return m.cuda()


def _setup(N, H, D, dtype, seed, weights, off=0, a_sizes=None, **feat_kw):
    """(fa, fb, rows_a (n_a, N), rows_b (n_a, n_b, N)); set A's sizes are unequal, the two cells of every column have different rows"""
    ts = _feats(N_A + N_B, seed, dtype, N, H, D, **feat_kw)
    fa, fb = tuple(t[:N_A].contiguous() for t in ts), tuple(t[N_A:].contiguous() for t in ts)
    ra = _rows(N, a_sizes or [N // 2 + 1, min(70, N - 3)], seed + 1, weights)
    cells = _cell_sizes(N, off)
    rb = _rows(N, [s for row in cells for s in row], seed + 2, weights).view(N_A, N_B, N)
    for j in range(N_B):
        assert not torch.equal(rb[0, j], rb[1, j]), j          # an implementation that reads rows_b[0][j] for every i must fail
    return fa, fb, ra, rb


def _pair_cell(tail, fa, fb, ra, rb, i, j, H, sim, **kw):
    """the pair tail of cell (i, j) as a 2-image call with that cell's two rows"""
    two = tuple(torch.cat([a[i:i + 1], b[j:j + 1]]) for a, b in zip(fa, fb))
    rows = torch.stack([ra[i], rb[i, j]]).contiguous()
    ia, ib = torch.tensor([0], dtype=torch.int32).cuda(), torch.tensor([1], dtype=torch.int32).cuda()
    return tail(*two, rows, ia, ib, H, sim, **kw)


def _forms(eng):
    """(weights?, the cell matrix, the matrix with rows per image, the pair tail)"""
    return ((False, eng.score_matrix_cell_regions, eng.score_matrix_regions, eng.pair_score_regions),
            (True, eng.score_matrix_cell_weights, eng.score_matrix_weights, eng.pair_score_weights))


# ---- 1. the pair tails per cell, to the bit ---------------------------------------------------------------------------------------------
def test_the_cell_sizes_cover_the_boundaries():
    for N in (256, 144, 64):
        seen = {s for off in (0, 3) for row in _cell_sizes(N, off) for s in row}
        assert seen == {s for s in (1, 63, 65, 128, 129, N - 1, N) if s <= N}, (N, seen)
        for off in (0, 3):
            c = _cell_sizes(N, off)
            assert all(c[0][j] != c[1][j] for j in range(N_B)), (N, off, c)


@pytest.mark.parametrize("N,H,D,dtype", CASES, ids=IDS)
@pytest.mark.parametrize("sim", ["cosine", "mse"])
def test_every_cell_equals_the_region_pair_tail(eng, N, H, D, dtype, sim):
    fa, fb, ma, mb = _setup(N, H, D, dtype, 100 + N + D, False)
    got, st, cnt = eng.score_matrix_cell_regions(fa, fb, ma, mb, H, sim, return_status=True, return_counts=True)
    assert got.shape == (N_A, N_B) and not st.any()
    assert cnt.tolist() == ma.sum(1).tolist() + mb.sum(2).flatten().tolist()
    for i in range(N_A):
        for j in range(N_B):
            want, wst = _pair_cell(eng.pair_score_regions, fa, fb, ma, mb, i, j, H, sim, return_status=True)
            assert torch.equal(got[i, j], want[0]) and int(wst) == 0, (i, j, got[i, j], want)


@pytest.mark.parametrize("N,H,D,dtype", CASES, ids=IDS)
@pytest.mark.parametrize("sim", ["cosine", "mse"])
def test_every_cell_equals_the_soft_pair_tail(eng, N, H, D, dtype, sim):
    fa, fb, wa, wb = _setup(N, H, D, dtype, 200 + N + D, True, off=3)
    got, st, sums = eng.score_matrix_cell_weights(fa, fb, wa, wb, H, sim, return_status=True, return_sums=True)
    assert got.shape == (N_A, N_B) and not st.any()
    assert sums.tolist() == wa.long().sum(1).tolist() + wb.long().sum(2).flatten().tolist()
    for i in range(N_A):
        for j in range(N_B):
            want, wst = _pair_cell(eng.pair_score_weights, fa, fb, wa, wb, i, j, H, sim, return_status=True)
            assert torch.equal(got[i, j], want[0]) and int(wst) == 0, (i, j, got[i, j], want)


# ---- 2. rows equal along i: the region / soft matrix; every row full: the score matrix ----------------------------------------------------
@pytest.mark.parametrize("N,H,D,dtype", [(256, 2, 160, torch.bfloat16), (144, 2, 72, torch.float32), (256, 4, 40, torch.float16),
                                         (64, 4, 32, torch.bfloat16)], ids=str)
def test_rows_equal_along_i_give_the_matrix_with_rows_per_image(eng, N, H, D, dtype):
    for weights, cell_matrix, matrix, _tail in _forms(eng):
        fa, fb, ra, rb = _setup(N, H, D, dtype, 300 + N + D, weights)
        per_image = rb[1].contiguous()                                               # (n_b, N)
        same = per_image.unsqueeze(0).expand(N_A, N_B, N).contiguous()
        for sim in ("cosine", "mse"):
            got, st, ext = cell_matrix(fa, fb, ra, same, H, sim, True, True)
            want, wst, wext = matrix(fa, fb, ra, per_image, H, sim, True, True)
            assert torch.equal(got, want) and torch.equal(st, wst), (weights, sim, got, want)
            assert ext.tolist() == wext[:N_A].tolist() + wext[N_A:].tolist() * N_A


@pytest.mark.parametrize("dtype,N,H,D", [(torch.float32, 256, 2, 160), (torch.float32, 144, 2, 72), (torch.bfloat16, 256, 4, 40),
                                         (torch.float16, 256, 4, 40)])
def test_full_rows_are_the_score_matrix(eng, dtype, N, H, D):
    """tests/test_gpu_region_matrix.py::test_full_masks_are_the_score_matrix's rule and cases (wherever score_matrix is the tiled
    kernel): bool ones and bytes of 255 through the region form, bytes of 255 through the soft form"""
    ts = _feats(N_A + N_B, 21 + N + D, dtype, N, H, D)
    fa, fb = tuple(t[:N_A].contiguous() for t in ts), tuple(t[N_A:].contiguous() for t in ts)
    ones = torch.ones(N_A, N_B, N, dtype=torch.bool, device="cuda")
    b255 = torch.full((N_A, N_B, N), 255, dtype=torch.uint8, device="cuda")
    for sim in ("cosine", "mse"):
        want, wst = eng.score_matrix(fa, fb, H, sim, return_status=True)
        for fn, rows in ((eng.score_matrix_cell_regions, ones), (eng.score_matrix_cell_regions, b255), (eng.score_matrix_cell_weights, b255)):
            got, st, ext = fn(fa, fb, rows[:, 0].contiguous(), rows, H, sim, True, True)
            assert torch.equal(got, want) and torch.equal(st, wst), (sim, fn.__name__, got, want)
            assert ext.tolist() == [N * (255 if fn is eng.score_matrix_cell_weights else 1)] * (N_A + N_A * N_B)


# ---- 3. float64, unequal per-cell regions -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda v: str(v)[6:])
@pytest.mark.parametrize("sim", ["cosine", "mse"])
def test_unequal_cell_regions_match_float64(eng, dtype, sim):
    """(256, 4, 40), the six cells with six different set-B sizes, both forms, against tests/_region64.py / tests/_soft64.py on the
    cell's two images and rows, under tests/test_gpu_region_matrix.py's _gate(dtype, False, sim); the features carry a channel mean
    for the reason test_unequal_regions_match_float64 gives there."""
    N, H, D = 256, 4, 40
    gate = _gate(dtype, False, sim)
    for weights, cell_matrix, _matrix, _tail in _forms(eng):
        fa, fb, ra, rb = _setup(N, H, D, dtype, 41 + N + D, weights, channel_mean=1.0)
        got, st = cell_matrix(fa, fb, ra, rb, H, sim, return_status=True)
        assert not st.any()
        ref = soft64 if weights else regions64
        errs = {}
        for i in range(N_A):
            for j in range(N_B):
                two = tuple(torch.cat([a[i:i + 1], b[j:j + 1]]) for a, b in zip(fa, fb))
                want = ref(*two, torch.stack([ra[i], rb[i, j]]), [0], [1], H, sim, dtype)[0]
                errs[(i, j)] = _score_err(float(got[i, j]), want, sim, dtype)
        print(f"cell {'weights' if weights else 'regions'} {str(dtype)[6:]} {sim}: largest err {max(errs.values()):.3e} gate {gate:.1e}")
        for c, e in errs.items():
            assert e <= gate, (weights, c, float(got[c]), e)


# ---- 4. empty rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 2, 160), (torch.float32, 144, 2, 72), (torch.float16, 64, 4, 32)])
def test_empty_rows_are_reported_in_their_cell_or_row_alone(eng, dtype, N, H, D):
    for weights, cell_matrix, _matrix, _tail in _forms(eng):
        fa, fb, ra, rb = _setup(N, H, D, dtype, 81, weights)
        for sim in ("cosine", "mse"):
            clean = cell_matrix(fa, fb, ra, rb, H, sim)
            one = rb.clone()
            one[1, 2] = 0                                                            # one empty cell row
            got, st, ext = cell_matrix(fa, fb, ra, one, H, sim, True, True)
            want_st = torch.zeros(N_A, N_B, dtype=torch.int32)
            want_st[1, 2] = 2
            assert torch.equal(st.cpu(), want_st) and ext[N_A + 1 * N_B + 2] == 0
            keep = want_st == 0
            assert bool(torch.isnan(got[1, 2])) and torch.equal(got.cpu()[keep], clean.cpu()[keep]), (weights, sim, got, clean)
            none_a = ra.clone()
            none_a[0] = 0                                                            # an empty mask_a[0]: row 0 alone
            got, st = cell_matrix(fa, fb, none_a, rb, H, sim, return_status=True)
            assert st.tolist() == [[2] * N_B, [0] * N_B]
            assert bool(torch.isnan(got[0]).all()) and torch.equal(got[1], clean[1]), (weights, sim, got, clean)
        got, st = cell_matrix(fa, fb, torch.zeros_like(ra), torch.zeros_like(rb), H, "cosine", return_status=True)      # every row empty
        assert bool(torch.isnan(got).all()) and bool((st == 2).all())


# ---- 5. nothing outside the rows is read into arithmetic --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 2, 160), (torch.float16, 256, 4, 40), (torch.float32, 144, 2, 72)])
def test_off_tokens_are_never_read(eng, dtype, N, H, D):
    """tests/test_gpu_region_matrix.py::test_off_region_rows_are_never_read's poison: the rows of a query off mask_a[i], and the rows
    of a gallery image that are off in every cell of its column"""
    for weights, cell_matrix, _matrix, _tail in _forms(eng):
        ts = _feats(N_A + N_B, 51, dtype, N, H, D)
        ra = _rows(N, [N // 2 + 1, 70], 5, weights)
        rb = _rows(N, [33, 65, 1, 40, 17, 63], 6, weights).view(N_A, N_B, N)
        off = torch.cat([ra == 0, ((rb != 0).sum(0) == 0)])                          # (n_a + n_b, N)
        assert bool(off.any(1).all())
        for sim in ("cosine", "mse"):
            clean = cell_matrix(tuple(t[:N_A].contiguous() for t in ts), tuple(t[N_A:].contiguous() for t in ts), ra, rb, H, sim)
            nan = tuple(t.clone() for t in ts)
            big = tuple(t.clone() for t in ts)
            for t in nan:
                t.transpose(1, 2)[off] = float("nan")              # (n, N, B, HD) view: every off row of every CFG half
            for t in big:
                rows = t.transpose(1, 2)
                fill = torch.full_like(rows[off], 65504.0)
                fill[0::3] = float("inf")
                fill[1::3] = float("-inf")
                rows[off] = fill
            for bad in (nan, big):
                assert not torch.isfinite(bad[0].float()).all()
                got, st = cell_matrix(tuple(t[:N_A].contiguous() for t in bad), tuple(t[N_A:].contiguous() for t in bad), ra, rb, H, sim,
                                      return_status=True)
                assert torch.equal(got, clean) and not st.any(), (weights, sim, got, clean, st)


# ---- 6. independence ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 2, 160), (torch.float16, 144, 2, 72), (torch.float32, 256, 4, 40)])
def test_a_cell_alone_a_repeat_and_two_streams(eng, dtype, N, H, D):
    for weights, cell_matrix, _matrix, _tail in _forms(eng):
        fa, fb, ra, rb = _setup(N, H, D, dtype, 71, weights)
        for sim in ("cosine", "mse"):
            r1 = cell_matrix(fa, fb, ra, rb, H, sim)
            assert torch.equal(r1, cell_matrix(fa, fb, ra, rb, H, sim))                                       # a repeat call
            for i in range(N_A):                                                                              # a cell alone
                for j in range(N_B):
                    one = cell_matrix(tuple(t[i:i + 1] for t in fa), tuple(t[j:j + 1] for t in fb), ra[i:i + 1], rb[i:i + 1, j:j + 1].contiguous(),
                                      H, sim)
                    assert torch.equal(one[0, 0], r1[i, j]), (weights, sim, i, j)
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]                                              # two streams
            torch.cuda.synchronize()
            res = []
            for s in streams:
                with torch.cuda.stream(s):
                    res.append(cell_matrix(fa, fb, ra, rb, H, sim))
            torch.cuda.synchronize()
            assert torch.equal(res[0], r1) and torch.equal(res[1], r1)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("form", ["regions", "weights"])
def test_refusals_enqueue_nothing(eng, form):
    """DSIM_ERR_WORKSPACE for a workspace one byte short of what the launcher needs (the query's answer less its 256 bytes of
    alignment slack; the pointer here is aligned), DSIM_ERR_INVALID with a workspace query of 0 for n_a = 0, a head dim outside the
    set and a bad dtype, DSIM_ERR_INVALID for a bad similarity and a NULL row array; the outputs keep their bytes in every case."""
    from diffsim_amd import _lib
    L = _lib.lib()
    N, H, D = 64, 4, 32
    weights = form == "weights"
    fa, fb, ra, rb = _setup(N, H, D, torch.bfloat16, 91, weights)
    ra8 = ra.view(torch.uint8)
    rb8 = rb.view(torch.uint8)
    query = getattr(L, f"dsim_score_matrix_cell_{form}_workspace_bytes")
    entry = getattr(L, f"dsim_score_matrix_cell_{form}")
    need = int(query(N_A, N_B, B, H, N, D, _lib.DSIM_BF16))
    assert need > 256
    # no image-sized slab per cell: set A's self outputs are the only feature-sized part
    assert need < 2 * N_A * B * N * H * D * 2 + (N_A + N_A * N_B) * (N * 8 + 1024) + N_A * N_B * 2 * B * H * 16 + 4096
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0

    def call(n_a=N_A, D_=D, dtype=_lib.DSIM_BF16, wsb=need, sim=0, null=()):
        out = torch.full((N_A, N_B), -7.0, device="cuda")
        status = torch.full((N_A, N_B), -7, dtype=torch.int32, device="cuda")
        rc = entry(_p(fa[0]), _p(fa[1]), _p(fa[2]), _p(ra8), n_a, _p(fb[0]), _p(fb[1]), _p(fb[2]), None if "rows_b" in null else _p(rb8), N_B,
                   B, H, N, D_, dtype, sim, _p(out), _p(status), None, _p(ws), wsb, None)
        torch.cuda.synchronize()
        return rc, out, status
    for shape in ((0, N_B, B, H, N, D, _lib.DSIM_BF16), (N_A, N_B, B, H, N, 24, _lib.DSIM_BF16), (N_A, N_B, B, H, N, D, 9),
                  (40000, 30000, B, H, N, D, _lib.DSIM_BF16), (N_A, N_B, 300, 300, N, D, _lib.DSIM_BF16),
                  (60000, 5000, 1, 1, 64, 16, _lib.DSIM_BF16)):
        assert query(*shape) == 0, shape
    for kw, text in ((dict(n_a=0), b"invalid"), (dict(D_=24), b"invalid"), (dict(dtype=9), b"invalid"), (dict(sim=2), b"invalid"),
                     (dict(null=("rows_b",)), b"invalid"), (dict(wsb=need - 257), b"workspace")):
        rc, out, status = call(**kw)
        assert rc != 0 and text in L.dsim_strerror(rc).lower(), (kw, rc)
        assert bool((out == -7.0).all()) and bool((status == -7).all()), kw
    rc, out, status = call(wsb=need - 256)                           # the same call with the workspace it needs
    want = (eng.score_matrix_cell_weights if weights else eng.score_matrix_cell_regions)(fa, fb, ra, rb, H)
    assert rc == 0 and torch.equal(out, want) and not status.any()
    # the Python entry's own checks: rows of the wrong extent or kind
    for bad_a, bad_b in ((ra[:1], rb), (ra, rb[0]), (ra, rb[:, :2].contiguous()), (ra, rb.transpose(0, 1))):
        with pytest.raises(_lib.DsimError):
            (eng.score_matrix_cell_weights if weights else eng.score_matrix_cell_regions)(fa, fb, bad_a, bad_b, H)
