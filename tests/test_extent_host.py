"""CPU checks of tests/_extent.py, the helpers the GPU extent tests rest on: the choice of M lands on the 2 GiB bound (exclusive)
and leaves a ragged last tile at every tile height of the plan table; the row chooser contains every row the method names, for M,
ldo and element sizes at and around the bound; and the periodic check, with the sentinel check, catches each planted defect on
small simulated buffers -- a row stored at its offset modulo the (simulated) wrap, a row dropped, a 16-byte piece exchanged
between periods, a sentinel overwritten -- and passes the clean buffer."""
import pytest
import torch

from tests import _extent as E

SENT = -12345.0
ROW_BYTES = [320 * 2, 328 * 2, 320 * 4, 328 * 4, 640 * 2, 1152 * 2, 1152 * 4, 1280 * 2, 1280 * 4, 128 * 2, 256 * 2, 960 * 2]


@pytest.mark.parametrize("rb", ROW_BYTES)
def test_bound_rows_lands_on_the_bound_with_a_ragged_last_tile(rb):
    M, refused = E.bound_rows(rb)
    assert M * rb < E.LIMIT and refused * rb >= E.LIMIT and (refused - 1) * rb < E.LIMIT
    assert refused - 1 == (E.LIMIT - 1) // rb                      # the issue's floor((0x7fffffff - 1) / (ldo es))
    assert 0 < refused - M <= 2                                     # lowered by at most one row
    for t in E.TILE_HEIGHTS:
        assert M % t != 0, (M, t)
    assert M * rb > E.LIMIT - 3 * rb


def test_bound_rows_with_gaps_and_copies():
    """out_split: N / out_split tensors `stride` bytes apart, stride = M row_bytes + gap; the launcher admits copies * stride below
    the limit"""
    rb, gap = 328 * 2, 1024
    M, refused = E.bound_rows(rb, fixed_bytes=gap, copies=3)
    assert 3 * (M * rb + gap) < E.LIMIT <= 3 * (refused * rb + gap)
    assert all(M % t for t in E.TILE_HEIGHTS)


def test_bound_images():
    for img in (64 * 64 * 320 * 2, 32 * 32 * 640 * 4, 196 * 320 * 2):
        B, refused = E.bound_images(img)
        assert B * img < E.LIMIT <= refused * img and refused == B + 1


@pytest.mark.parametrize("es", [2, 4])
@pytest.mark.parametrize("ldo", [320, 328, 1152, 1280])
@pytest.mark.parametrize("dm", [0, -1, -77, -4096])
@pytest.mark.parametrize("tile", [128, 256, 512])
def test_required_rows_contains_every_named_row(es, ldo, dm, tile):
    c0 = 320
    M = E.bound_rows(ldo * es)[0] + dm
    rbs = (c0 * es, ldo * es)
    rows = set(E.required_rows(M, tile, rbs, n_random=64, seed=1).tolist())
    assert 0 in rows and M - 1 in rows
    last0 = (M - 1) // tile * tile
    assert all(r in rows for r in range(last0, M)), "the last M tile, up to its last valid row"
    for rb in rbs:
        for b in (1 << 30, (1 << 31) - tile * rb):
            r = b // rb
            assert r * rb <= b < (r + 1) * rb
            for v in (r - 1, r, r + 1):
                assert v in rows or not (0 <= v < M), (rb, b, v)
    assert len(rows) >= 64 and len(rows) <= 64 + 2 + tile + 12
    assert min(rows) >= 0 and max(rows) < M
    assert rows == set(E.required_rows(M, tile, rbs, n_random=64, seed=1).tolist())


# ---- the periodic check on simulated buffers ----------------------------------------------------------------------------------------
P, LDO, COLS, M_SIM, NOUT, GAP = 16, 24, 16, 16 * 9 + 5, 2, 32      # 9 whole periods and a ragged tenth; 8 pad columns; two tensors
WRAP = 1 << 12               # the simulated offset width: a "kernel" with too narrow an offset stores row r at (r row_bytes) mod WRAP


def _simulate(dtype, defect=None):
    """what a correct kernel leaves for a periodic operand (out[r] = 2 A[r mod P] + column), in the GPU tests' buffer layout, with
    one planted defect"""
    g = torch.Generator().manual_seed(5)
    base = torch.randn(P, COLS, generator=g).to(dtype)
    a = E.periodic_rows(base, M_SIM)
    n, per = E.out_layout(M_SIM, LDO, NOUT, GAP)
    out = torch.full((n,), SENT, dtype=dtype)
    es = out.element_size()
    for j in range(NOUT):
        blk = out[j * per:j * per + M_SIM * LDO].view(M_SIM, LDO)
        blk[:, :COLS] = (a.float() * 2 + j).to(dtype)
    blk = out[:M_SIM * LDO].view(M_SIM, LDO)
    if defect == "row_wrapped":
        r = M_SIM - 3                                                   # its byte offset lies beyond WRAP
        assert r * LDO * es >= WRAP
        dst = (r * LDO * es) % WRAP // es
        row = blk[r, :COLS].clone()
        blk[r, :COLS] = SENT                                            # never written where it belongs
        out[dst:dst + COLS] = row                                       # ... but on top of an early row
    elif defect == "row_dropped":
        blk[5 * P + 3, :COLS] = SENT
    elif defect == "row_dropped_as_neighbour":                          # a dropped store that leaves stale data of the row before
        blk[5 * P + 3, :COLS] = blk[5 * P + 2, :COLS].clone()
    elif defect == "piece_swapped":
        k = 16 // es                                                    # a 16-byte piece
        a_, b_ = blk[2 * P + 1, :k].clone(), blk[6 * P + 9, k:2 * k].clone()
        blk[2 * P + 1, :k], blk[6 * P + 9, k:2 * k] = b_, a_
    elif defect == "sentinel_pad":
        blk[7 * P + 2, COLS + 1] = 1.0
    elif defect == "sentinel_gap":
        out[M_SIM * LDO + 3] = 1.0
    elif defect == "sentinel_guard":
        out[NOUT * per + LDO] = 1.0
    else:
        assert defect is None
    return out, per


def _verdict(out, per):
    """(periodic, sentinels): what the GPU tests assert, on every out_split tensor"""
    ok = all(E.periodic_ok(out[j * per:j * per + M_SIM * LDO], M_SIM, LDO, P, chunk=4) for j in range(NOUT))
    return ok, E.sentinels_ok(out, M_SIM, LDO, COLS, NOUT, per, SENT)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_clean_buffer_passes(dtype):
    out, per = _simulate(dtype)
    assert _verdict(out, per) == (True, None)
    assert E.periodic_bad_rows(out[:M_SIM * LDO], M_SIM, LDO, P) == []


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("defect", ["row_wrapped", "row_dropped", "row_dropped_as_neighbour", "piece_swapped"])
def test_periodic_check_catches(defect, dtype):
    out, per = _simulate(dtype, defect)
    ok, _ = _verdict(out, per)
    assert not ok, defect
    bad = E.periodic_bad_rows(out[:M_SIM * LDO], M_SIM, LDO, P)
    assert bad, defect
    want = {"row_wrapped": M_SIM - 3, "row_dropped": 5 * P + 3, "row_dropped_as_neighbour": 5 * P + 3, "piece_swapped": 2 * P + 1}[defect]
    assert want in bad, (defect, bad)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("defect,where", [("sentinel_pad", "columns"), ("sentinel_gap", "gap"), ("sentinel_guard", "guard")])
def test_sentinel_check_catches(defect, where, dtype):
    out, per = _simulate(dtype, defect)
    _, s = _verdict(out, per)
    assert s is not None and where in s, (defect, s)


def test_a_defect_in_period_zero_alone_is_left_to_the_float64_rows():
    """the periodic check compares with period 0, so a wrong period 0 shows as EVERY other period differing -- and a defect that
    repeats in every period is what the float64 check of period 0 is for: required_rows() and _gemm64.row_subset cover it"""
    out, per = _simulate(torch.float32)
    out[:M_SIM * LDO].view(M_SIM, LDO)[3, 2] += 1.0
    assert not E.periodic_ok(out[:M_SIM * LDO], M_SIM, LDO, P)
    assert len(E.periodic_bad_rows(out[:M_SIM * LDO], M_SIM, LDO, P, limit=100)) == M_SIM // P


def test_periodic_rows_and_odd_alignment():
    base = torch.arange(5 * 3, dtype=torch.float32).view(5, 3).to(torch.bfloat16)
    a = E.periodic_rows(base, 17)
    assert all(torch.equal(a[r], base[r % 5]) for r in range(17))
    flat = torch.cat([torch.zeros(1, dtype=torch.bfloat16), a.flatten()])[1:]      # a 2-byte aligned start, 6-byte rows
    assert E.periodic_ok(flat, 17, 3, 5)
    flat[16 * 3 + 1] = 99.0
    assert not E.periodic_ok(flat, 17, 3, 5)
