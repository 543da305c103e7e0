"""Region alignments on the GPU (csrc/region_maps.hip behind dsim_pair_align_regions; engine.pair_align_regions), through the C ABI:
to the bit against dsim_pair_align on physically compacted tensors and, with full masks, against dsim_pair_align itself; against the
float64 restatement and per-entry bound of tests/_regionmap64.py (tests/_align64.py on the gathered rows); and for what the header
promises: the off values at the off query tokens, zeros of attn outside R_a x R_b, nothing outside a region read, full-grid
coordinates, a pair independent of its neighbours, an empty region reported.

Gates are test_gpu_align's: attn within 2e-5 x the reference row's maximum (ordinary logits) or within the _align64 bound (logits
scaled by 14); match / weight / expect by the rules of its test_match_is_a_near_maximiser_with_its_weight_and_expectation, restricted
to the key region.
REGION_ALIGN_FIRST_RUN below: the largest err / gate of the first MI355X run per family (recorded, not used)."""
import ctypes
import functools

import pytest
import torch

from tests import _align64 as A
from tests import _regionmap64 as R

pytestmark = pytest.mark.gpu

B = A.B
# first MI355X run, largest attn err / gate over the cases of test_unequal_regions_match_float64: ordinary family (gate 2e-5 x row
# maximum) 0.017 at fp32 (256, 8, 160), the 16-bit modes <= 0.014; scaled family (_align64 bound) 0.060 at fp32 (256, 4, 40), the 16-bit
# modes <= 0.024.  Every gate held, so none was re-derived
REGION_ALIGN_FIRST_RUN = {"ordinary": 0.017, "scaled": 0.060}
FAMILIES = {"ordinary": 1.0, "scaled": 14.0}
NAMES = ("match", "weight", "expect", "attn", "status")


def _idx(xs):
    return torch.tensor(list(xs), dtype=torch.int32).cuda()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _masks(N, sizes, seed):
    """(len(sizes), N) bool on the CPU: image i's region is sizes[i] tokens at seeded positions"""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(len(sizes), N, dtype=torch.bool)
    for i, r in enumerate(sizes):
        m[i, torch.randperm(N, generator=g)[:r]] = True
    return m


def _grid_w(N):
    """a grid width that divides N: the square's where N is one, else the largest divisor up to sqrt(N)"""
    w = int(N ** 0.5)
    while N % w:
        w -= 1
    return w


def call(q, k, mask, ia, ib, H, grid_w, want=NAMES, ws_bytes=None, counts=False):
    """dsim_pair_align_regions through the C ABI on device tensors q, k [n][B][N][H*D], mask (n, N); (rc, {name: tensor}) with the
    outputs named in want (and counts)"""
    from diffsim_amd import _lib
    from diffsim_amd.engine import _TORCH2DSIM
    L = _lib.lib()
    n, (nf, Bc, N, HD) = ia.numel(), q.shape
    D = HD // H
    o = {"match": torch.full((n, 2, N), -7, dtype=torch.int32, device="cuda"),
         "weight": torch.full((n, 2, N), -7.0, device="cuda"),
         "expect": torch.full((n, 2, N, 2), -7.0, device="cuda"),
         "attn": torch.full((n, 2, N, N), -7.0, device="cuda"),
         "status": torch.full((n,), -7, dtype=torch.int32, device="cuda")}
    o = {name: t for name, t in o.items() if name in want}
    if counts:
        o["counts"] = torch.full((nf,), -7, dtype=torch.int32, device="cuda")
    m8 = mask.cuda().contiguous().view(torch.uint8) if mask.dtype == torch.bool else mask.cuda().contiguous()
    need = int(L.dsim_pair_align_regions_workspace_bytes(nf, n, Bc, H, N, D))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    rc = L.dsim_pair_align_regions(_p(q), _p(k), _p(m8), nf, _p(ia), _p(ib), n, Bc, H, N, D, _TORCH2DSIM[q.dtype], grid_w,
                                   _p(o.get("match")), _p(o.get("weight")), _p(o.get("expect")), _p(o.get("attn")), _p(o.get("status")),
                                   _p(o.get("counts")), _p(ws), need if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    return rc, o


def whole(q, k, ia, ib, H, grid_w, want=NAMES):
    """dsim_pair_align (tests/test_gpu_align.call)"""
    from tests.test_gpu_align import call as call_whole
    return call_whole(q, k, ia, ib, H, grid_w, want=want)


def _compact(ts, mask):
    rows = R.rows_of(mask)
    return tuple(torch.stack([t[i].index_select(1, rows[i].to(t.device)) for i in range(t.shape[0])]).contiguous() for t in ts)


# ---- 1. dsim_pair_align on compacted tensors, to the bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 63, 64, 65, 127, 128, 129, 255])
@pytest.mark.parametrize("D", [160, 40, 72])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["float32", "bfloat16", "float16"])
def test_equals_the_alignment_of_the_compacted_tensors(dtype, D, r):
    """Two images with regions of r tokens at different positions inside N = 256: weight and the R_a x R_b block of attn are
    dsim_pair_align's on the (n, B, r, H*D) tensors of the regions' rows, bit for bit; match is its match mapped through the key
    image's list; everything else holds the off values."""
    N, H = 256, 2
    q, k = (t.cuda() for t in A.feats(2, 100 + r + D, dtype, N, H, D))
    mask = _masks(N, [r, r], 7 * r + D)
    assert not torch.equal(mask[0], mask[1])
    rows = [x.cuda() for x in R.rows_of(mask)]
    cq, ck = _compact((q, k), mask)
    pairs = [(0, 1), (1, 0), (0, 0)]
    ia, ib = _idx(a for a, _ in pairs), _idx(b for _, b in pairs)
    rc, o = call(q, k, mask, ia, ib, H, 16)
    assert rc == 0 and o["status"].tolist() == [0, 0, 0]
    rc, w = whole(cq, ck, ia, ib, H, 1)                              # (r tokens form no grid: a column, its expect is not compared)
    assert rc == 0
    md = mask.cuda()
    for p, pr in enumerate(pairs):
        for d in range(2):
            iq, ix = pr[d], pr[1 - d]
            assert torch.equal(o["weight"][p, d, rows[iq]], w["weight"][p, d]), (p, d)
            assert torch.equal(o["match"][p, d, rows[iq]].long(), rows[ix][w["match"][p, d].long()]), (p, d)
            assert torch.equal(o["attn"][p, d][rows[iq]][:, rows[ix]], w["attn"][p, d]), (p, d)
            outside = ~(md[iq][:, None] & md[ix][None, :])
            assert not o["attn"][p, d][outside].any()
            off = ~md[iq]
            assert (o["match"][p, d][off] == -1).all() and not o["weight"][p, d][off].any() and (o["expect"][p, d][off] == -1).all()


# ---- 2. full regions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,D", [(256, 8, 160), (144, 2, 72), (196, 8, 72), (49, 2, 16)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["float32", "bfloat16", "float16"])
def test_full_regions_are_the_whole_image_alignment(dtype, N, H, D):
    q, k = (t.cuda() for t in A.feats(3, 21 + N + D, dtype, N, H, D))
    ia, ib = _idx([0, 1, 2, 1]), _idx([1, 2, 0, 1])
    w = _grid_w(N)
    rc, want = whole(q, k, ia, ib, H, w)
    assert rc == 0
    for mask in (torch.ones(3, N, dtype=torch.bool), torch.full((3, N), 255, dtype=torch.uint8)):
        rc, got = call(q, k, mask, ia, ib, H, w, counts=True)
        assert rc == 0 and got["counts"].tolist() == [N] * 3
        for name in NAMES:
            assert torch.equal(got[name], want[name]), name


# ---- 3. float64, unequal regions ------------------------------------------------------------------------------------------------------
def _sizes(N):
    return [N, 129 if N == 256 else N // 2 + 1, 64 if N == 256 else N // 4, 1]


CASES = [(N, H, D, dt, _sizes(N), ((0, 1), (1, 2), (2, 3), (3, 0), (1, 1)))
         for N, H, D in ((256, 8, 160), (256, 4, 40), (196, 8, 72), (64, 4, 32)) for dt in (torch.float32, torch.bfloat16, torch.float16)]
CASES.append((1024, 8, 80, torch.bfloat16, [700, 130], ((0, 1),)))          # several query tiles, early-leaving workgroups
IDS = [f"{N}-{H}-{D}-{str(dt)[6:]}" for N, H, D, dt, _, _ in CASES]


@functools.lru_cache(maxsize=None)
def _case(N, H, D, dtype, sizes, pairs, family):
    """(q, k on the device, mask, Pm64, bound64, kernel outputs on the CPU) of one case, computed once"""
    q, k = A.feats(len(sizes), 41 + N + D, dtype, N, H, D, logit_scale=FAMILIES[family])
    mask = _masks(N, list(sizes), N + D)
    Pm, bound = R.region_align64(q, k, mask, pairs, H)
    qd, kd = q.cuda(), k.cuda()
    rc, o = call(qd, kd, mask, _idx(p[0] for p in pairs), _idx(p[1] for p in pairs), H, _grid_w(N), counts=True)
    assert rc == 0
    return qd, kd, mask, Pm, bound, {name: t.cpu() for name, t in o.items()}


def _gate(Pm, bound, family):
    """test_gpu_align._gate: 2e-5 x the row maximum (ordinary), the bound (scaled)"""
    return A.ORDINARY_REL * Pm.max(-1, keepdim=True).values.expand_as(Pm) if family == "ordinary" else bound


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("N,H,D,dtype,sizes,pairs", CASES, ids=IDS)
def test_unequal_regions_match_float64(N, H, D, dtype, sizes, pairs, family):
    _, _, mask, Pm, bound, o = _case(N, H, D, dtype, tuple(sizes), pairs, family)
    assert o["status"].tolist() == [0] * len(pairs) and o["counts"].tolist() == list(sizes)
    gate = _gate(Pm, bound, family)
    err = (o["attn"].double() - Pm).abs()
    inside = torch.stack([torch.stack([mask[pr[d]][:, None] & mask[pr[1 - d]][None, :] for d in range(2)]) for pr in pairs])
    assert not o["attn"][~inside].any()                              # exact zeros outside R_a x R_b
    ratio = (err[inside] / gate[inside]).max().item()
    print(f"{str(dtype)[6:]} N={N} H={H} D={D} {family}: max err/gate {ratio:.3f}")
    assert ratio <= 1.0, ratio
    # rows of the region sum to one
    rows = R.rows_of(mask)
    w = _grid_w(N)
    for p, pr in enumerate(pairs):
        for d in range(2):
            rq, rk = rows[pr[d]], rows[pr[1 - d]]
            attn = o["attn"][p, d].double()
            assert ((attn[rq].sum(-1) - 1).abs() <= (len(rk) + 64) * 2.0 ** -23).all()
            # match, weight, expect: test_gpu_align's rules over the key region
            match = o["match"][p, d].long()
            on_q = torch.zeros(N, dtype=torch.bool)
            on_q[rq] = True
            assert (match[~on_q] == -1).all() and not o["weight"][p, d][~on_q].any() and (o["expect"][p, d][~on_q] == -1).all()
            mq = match[rq]
            assert mask[pr[1 - d]][mq].all()                         # a match is a token of the key region
            P, G = Pm[p, d][rq], gate[p, d][rq]
            top, jmax = P.max(-1)
            at = P.gather(-1, mq[:, None])[:, 0]
            g_at, g_top = G.gather(-1, mq[:, None])[:, 0], G.gather(-1, jmax[:, None])[:, 0]
            tau = 2 * torch.maximum(g_at, g_top) / top
            assert (at >= (1 - tau) * top).all(), ((top - at) / top).max().item()
            assert ((o["weight"][p, d][rq].double() - at).abs() <= g_at).all()
            assert torch.equal(o["weight"][p, d][rq], o["attn"][p, d][rq].gather(-1, mq[:, None])[:, 0])
            j = torch.arange(N, dtype=torch.float64)
            coords = torch.stack([torch.div(j, w, rounding_mode="floor"), j % w], -1)
            want = attn[rq] @ coords
            assert ((o["expect"][p, d][rq].double() - want).abs() <= (len(rk) / 2 + 2) * A.U32 * want + 1e-30).all()


# ---- 4. nothing outside a region is read into arithmetic ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 2, 160), (torch.float16, 200, 4, 40), (torch.float32, 144, 2, 72)])
def test_off_region_rows_are_never_read(dtype, N, H, D):
    q, k = (t.cuda() for t in A.feats(3, 51, dtype, N, H, D))
    mask = _masks(N, [N // 2 + 1, 70, 33], 5)
    ia, ib = _idx([0, 1, 2]), _idx([1, 2, 0])
    w = _grid_w(N)
    rc, clean = call(q, k, mask, ia, ib, H, w)
    assert rc == 0
    q2, k2 = q.clone(), k.clone()
    for t in (q2, k2):
        t.transpose(1, 2)[~mask.cuda()] = float("nan")
    assert not torch.isfinite(q2.float()).all()
    rc, got = call(q2, k2, mask, ia, ib, H, w)
    assert rc == 0 and got["status"].tolist() == [0, 0, 0]
    for name in NAMES:
        assert torch.equal(got[name], clean[name]), name


# ---- 5. placement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,H,D", [(torch.bfloat16, 2, 160), (torch.float16, 2, 72), (torch.float32, 4, 40)])
def test_match_and_expect_follow_the_full_grid_coordinates(dtype, H, D):
    """The same region rows at other positions of N = 256 (16 wide) and of N = 512 (32 wide): weight and the attn block are
    bit-identical, match is the same key position's token, and expect is the attn row against that placement's coordinates."""
    sizes = [100, 77, 130]
    g = torch.Generator().manual_seed(61)
    vals = [tuple((torch.randn(B, r, H * D, generator=g) * (0.5 + j)).to(dtype) for j in range(2)) for r in sizes]
    pairs = [(0, 1), (1, 2), (2, 0)]
    ia, ib = _idx(a for a, _ in pairs), _idx(b for _, b in pairs)
    res = []
    for N, w, seed in ((256, 16, 1), (256, 16, 2), (512, 32, 3)):
        mask = _masks(N, sizes, seed)
        rows = R.rows_of(mask)
        q, k = (t.cuda() for t in A.feats(3, seed, dtype, N, H, D))
        for i in range(3):
            for t, x in zip((q, k), vals[i]):
                t[i].index_copy_(1, rows[i].cuda(), x.cuda())
        rc, o = call(q, k, mask, ia, ib, H, w)
        assert rc == 0 and o["status"].tolist() == [0, 0, 0]
        o = {n: t.cpu() for n, t in o.items()}
        per = []
        for p, pr in enumerate(pairs):
            for d in range(2):
                rq, rk = rows[pr[d]], rows[pr[1 - d]]
                block = o["attn"][p, d][rq][:, rk]
                pos = torch.searchsorted(rk, o["match"][p, d][rq].long())                 # the match as a key position
                assert torch.equal(rk[pos], o["match"][p, d][rq].long())
                coords = torch.stack([torch.div(rk, w, rounding_mode="floor"), rk % w], -1).double()
                want = block.double() @ coords
                got = o["expect"][p, d][rq].double()
                assert ((got - want).abs() <= (len(rk) / 2 + 2) * A.U32 * want + 1e-30).all()
                per.append((o["weight"][p, d][rq], block, pos))
        res.append(per)
    for other in res[1:]:
        for (w0, b0, p0), (w1, b1, p1) in zip(res[0], other):
            assert torch.equal(w0, w1) and torch.equal(b0, b1) and torch.equal(p0, p1)


# ---- 6. invariance and ties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,D,dtype", [(64, 4, 32, torch.float32), (196, 8, 72, torch.float16), (256, 8, 160, torch.bfloat16)])
def test_deterministic_batch_invariant_swap_symmetric_mask_byte_and_output_independent(N, H, D, dtype):
    sizes, pairs = tuple(_sizes(N)), ((0, 1), (1, 2), (2, 3), (3, 0), (1, 1))
    qd, kd, mask, _, _, first = _case(N, H, D, dtype, sizes, pairs, "ordinary")
    ia, ib = _idx(p[0] for p in pairs), _idx(p[1] for p in pairs)
    w = _grid_w(N)
    rc, again = call(qd, kd, mask, ia, ib, H, w)
    assert rc == 0 and all(torch.equal(again[n].cpu(), first[n]) for n in NAMES)            # repeat calls
    for p in range(len(pairs)):                                                             # n pairs == n single-pair calls
        rc, one = call(qd, kd, mask, ia[p:p + 1].clone(), ib[p:p + 1].clone(), H, w)
        assert rc == 0 and all(torch.equal(one[n][0].cpu(), first[n][p]) for n in NAMES)
    rc, sw = call(qd, kd, mask, ib, ia, H, w)                                               # swapping (a, b) swaps the directions
    assert rc == 0 and all(torch.equal(sw[n].cpu(), first[n].flip(1)) for n in NAMES[:4]) and torch.equal(sw["status"].cpu(), first["status"])
    for m in (mask.to(torch.uint8) * 255, mask.to(torch.uint8) * 3):                        # any non-zero byte is on
        rc, other = call(qd, kd, m, ia, ib, H, w)
        assert rc == 0 and all(torch.equal(other[n].cpu(), first[n]) for n in NAMES)
    for n in NAMES:                                                                         # any subset may be NULL
        rc, only = call(qd, kd, mask, ia, ib, H, w, want=(n,))
        assert rc == 0 and torch.equal(only[n].cpu(), first[n]), n
    rc, lean = call(qd, kd, mask, ia, ib, H, w, want=("match", "weight", "expect"))
    assert rc == 0 and all(torch.equal(lean[n].cpu(), first[n]) for n in lean)
    rc, none = call(qd, kd, mask, ia, ib, H, w, want=())
    assert rc == 0


@pytest.mark.parametrize("N,H,D,dtype,j1,j2", [(196, 8, 72, torch.float16, 5, 150), (256, 8, 160, torch.bfloat16, 3, 20),
                                               (64, 4, 32, torch.float32, 8, 17)])
def test_identical_key_rows_inside_the_region_tie_to_the_lower_token(N, H, D, dtype, j1, j2):
    """test_gpu_align's tie case with both doubled key rows inside R_b and off rows between them"""
    q, k = A.feats(2, 5 + N, dtype, N, H, D)
    k[1, :, j1] = (3.0 * q[0, :, 0].float()).to(dtype)
    k[1, :, j2] = k[1, :, j1]
    q[0, :, 1:4] = q[0, :, 0:1]
    mask = _masks(N, [N // 2, N // 2], 3)
    mask[0, :4] = True
    mask[1, j1] = mask[1, j2] = True
    mask[1, j1 + 1] = False
    rc, o = call(q.cuda(), k.cuda(), mask, _idx([0]), _idx([1]), H, _grid_w(N))
    assert rc == 0
    assert torch.equal(o["attn"][0, 0, :, j1], o["attn"][0, 0, :, j2])
    assert not (o["match"][0, 0] == j2).any()
    assert o["match"][0, 0, :4].tolist() == [j1] * 4
    assert o["weight"][0, 0, 0].item() == o["attn"][0, 0, 0, j2].item()


# ---- 7. empty region, non-finite features ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float32, 144, 2, 72), (torch.float16, 64, 4, 32)])
def test_an_empty_region_is_reported_and_leaves_the_others(dtype, N, H, D):
    q, k = (t.cuda() for t in A.feats(4, 81, dtype, N, H, D))
    mask = _masks(N, [N // 2, 40, 17, N], 4)
    ia, ib = _idx([0, 1, 2, 3, 2]), _idx([1, 2, 3, 0, 2])
    w = _grid_w(N)
    rc, clean = call(q, k, mask, ia, ib, H, w)
    assert rc == 0 and clean["status"].tolist() == [0] * 5
    m2 = mask.clone()
    m2[2] = False
    rc, got = call(q, k, m2, ia, ib, H, w, counts=True)
    assert rc == 0 and got["status"].tolist() == [0, 2, 2, 0, 2] and got["counts"].tolist() == [N // 2, 40, 0, N]
    for p in (1, 2, 4):
        assert (got["match"][p] == -1).all() and not got["weight"][p].any() and (got["expect"][p] == -1).all() and not got["attn"][p].any()
    for name in NAMES[:4]:
        assert torch.equal(got[name][[0, 3]], clean[name][[0, 3]]), name


@pytest.mark.parametrize("N,H,D,dtype", [(196, 8, 72, torch.float16), (64, 4, 32, torch.float32)])
def test_a_nan_key_flags_exactly_the_pairs_with_that_image(N, H, D, dtype):
    sizes, pairs = tuple(_sizes(N)), ((0, 1), (1, 2), (2, 3), (3, 0), (1, 1))
    qd, kd, mask, _, _, first = _case(N, H, D, dtype, sizes, pairs, "ordinary")
    k2 = kd.clone()
    k2[2, 1, int(torch.nonzero(mask[2])[3]), 5] = float("nan")          # an ON row of image 2
    rc, o = call(qd, k2, mask, _idx(p[0] for p in pairs), _idx(p[1] for p in pairs), H, _grid_w(N))
    assert rc == 0
    assert o["status"].tolist() == [1 if 2 in p else 0 for p in pairs] == [0, 1, 1, 0, 0]
    for n in ("match", "weight", "expect", "attn"):
        assert torch.equal(o[n][[0, 3, 4]].cpu(), first[n][[0, 3, 4]]), n


# ---- 8. error codes ---------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    from diffsim_amd import _lib
    L = _lib.lib()
    N, H, D = 64, 4, 32
    q, k = (t.cuda() for t in A.feats(2, 1, torch.bfloat16, N, H, D))
    mask = _masks(N, [30, 20], 1)
    ia, ib = _idx([0]), _idx([1])
    assert L.dsim_pair_align_regions_workspace_bytes(2, 1, B, H, N, D) >= 2 * N * 4 + 2 * 4 + 2 * B * H * N * 8
    assert L.dsim_pair_align_regions_workspace_bytes(2, 0, B, H, N, D) == 0                    # n_pairs < 1
    assert L.dsim_pair_align_regions_workspace_bytes(0, 1, B, H, N, D) == 0                    # n_feat < 1
    assert L.dsim_pair_align_regions_workspace_bytes(2, 1, B, H, N, 24) == 0                   # a head dim outside DSIM_FOR_EACH_D
    need = int(L.dsim_pair_align_regions_workspace_bytes(2, 1, B, H, N, D))
    rc, _ = call(q, k, mask, ia, ib, H, 8, ws_bytes=need // 2)
    assert rc != 0 and b"workspace" in L.dsim_strerror(rc).lower()
    for w in (7, 0):                                                                            # 7 does not divide 64
        rc, _ = call(q, k, mask, ia, ib, H, w)
        assert rc != 0 and b"invalid" in L.dsim_strerror(rc).lower()
    rc, o = call(q, k, mask, ia, ib, H, 16)                                                     # any divisor is a grid: 4 x 16
    assert rc == 0 and o["expect"][..., 1].max().item() <= 15.0 and o["expect"][..., 0].max().item() <= 3.0
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    m = torch.empty(2 * N, dtype=torch.int32, device="cuda")
    m8 = mask.cuda().view(torch.uint8)

    def raw(q_=q, mask_=m8, n=1, d=D, ws_=ws, n_feat=2):
        return L.dsim_pair_align_regions(_p(q_), _p(k), _p(mask_), n_feat, _p(ia), _p(ib), n, B, H, N, d, _lib.DSIM_BF16, 8, _p(m), None,
                                         None, None, None, None, _p(ws_), 1 << 20, None)
    assert raw() == 0
    torch.cuda.synchronize()
    for kw in ({"q_": None}, {"mask_": None}, {"ws_": None}, {"n": 0}, {"d": 24}, {"n_feat": 0}):
        rc = raw(**kw)
        assert rc != 0 and b"invalid" in L.dsim_strerror(rc).lower(), kw
    # an attn of 2 GiB or more is refused: one pair of 16384 tokens is 2 x 16384^2 x 4 B = 2 GiB exactly.  Every buffer has its
    # true size and the workspace its true byte count, so that nothing could be written out of bounds if the call went through
    N2, H2, D2 = 16384, 1, 16
    q2 = torch.zeros(2, B, N2, H2 * D2, dtype=torch.bfloat16, device="cuda")
    mask2 = torch.ones(2, N2, dtype=torch.uint8, device="cuda")
    attn = torch.empty((1, 2, N2, N2), dtype=torch.float32, device="cuda")
    assert attn.numel() * 4 == 1 << 31
    need = int(L.dsim_pair_align_regions_workspace_bytes(2, 1, B, H2, N2, D2))
    ws2 = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = L.dsim_pair_align_regions(_p(q2), _p(q2), _p(mask2), 2, _p(ia), _p(ib), 1, B, H2, N2, D2, _lib.DSIM_BF16, 128, None, None, None,
                                   _p(attn), None, None, _p(ws2), need, None)
    torch.cuda.synchronize()
    assert rc != 0 and b"invalid" in L.dsim_strerror(rc).lower()


def test_engine_pair_align_regions_wraps_the_call():
    from diffsim_amd import _lib, engine
    N, H, D = 64, 4, 32
    sizes, pairs = tuple(_sizes(N)), ((0, 1), (1, 2), (2, 3), (3, 0), (1, 1))
    qd, kd, mask, _, _, first = _case(N, H, D, torch.float32, sizes, pairs, "ordinary")
    ia, ib = _idx(p[0] for p in pairs), _idx(p[1] for p in pairs)
    md = mask.cuda()
    m, w, e = engine.pair_align_regions(qd, kd, md, ia, ib, H)                      # grid_w None: the square grid
    assert m.dtype == torch.int32 and m.shape == (5, 2, N) and e.shape == (5, 2, N, 2)
    assert torch.equal(m.cpu(), first["match"]) and torch.equal(w.cpu(), first["weight"]) and torch.equal(e.cpu(), first["expect"])
    m, w, e, a, st, cnt = engine.pair_align_regions(qd, kd, md, ia, ib, H, 8, return_attention=True, return_status=True,
                                                    return_counts=True)
    assert torch.equal(a.cpu(), first["attn"]) and st.tolist() == [0] * 5 and cnt.tolist() == list(sizes)
    with pytest.raises(_lib.DsimError):
        engine.pair_align_regions(qd, kd, md[:2], ia, ib, H)
    with pytest.raises(_lib.DsimError):
        engine.pair_align_regions(qd, kd.half(), md, ia, ib, H)
