"""Soft region alignments (dsim_pair_align_weights / engine.pair_align_weights): the region alignments with ln(weight) of each key
added to its logit.  Checked to the bit against engine.pair_align_regions where every byte is 0 or 255, against the float64
restatement tests/_softmap64.py by tests/_align64.py's rules (attn entry by entry under the bound, match a near-maximiser, weight and
expect from the kernel's own attn), and for what the header promises: attn rows are probability rows over the listed keys, weights
are multiplicities of keys, ties go to the lower token, an image without weight is reported.

THE WIDENED BOUND (tests/_softmap64.py has it term by term).  tests/_align64.py bounds a numerator's relative error by
rho = a + 2 u32 gap + 2^-23: the f32 accumulation of the logit, the two roundings of the scaled exponent argument (in natural units
each u32 |arg|, |arg| = gap), and the exponential.  The soft kernels compute exp2(fma(s, c, -m c) + lb) with m the raw maximum and
lb = log2(byte / 255) in [-7.995, 0] from an f32 table: one more f32 rounding, of an argument whose magnitude is at most 8 larger
in log2 units than the unbiased one -- u32 (gap + 8 ln 2) in natural units -- and the rounding of the table entry itself,
u32 8 ln 2.  So rho = a + 3 u32 gap + 16 ln 2 u32 + 2^-23, gap being the raw gap; everything else is _align64's, with the key
count's tiles.  Nothing is fitted to what the kernels return.

Recorded, not used -- the first MI355X run's largest attn err / bound per dtype over test_general_bytes_match_float64:

    dtype      err / bound
    float32    0.030
    bfloat16   0.023
    float16    0.020
"""
import pytest
import torch

from tests import _align64 as A
from tests._softmap64 import rows_of, soft_align64
from tests._tail64 import heads64
from tests.test_gpu_soft_regions import DTYPES, _feats, _idx, _poison, _sizes, _weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


def _grid_w(N):
    return {256: 16, 196: 14, 144: 12, 64: 8, 128: 16}[N]


# ---- 1. bytes 0 / 255 are the region alignments, bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 63, 64, 65, 127, 128, 129, 255])
@pytest.mark.parametrize("H,D", [(2, 160), (4, 40), (2, 72)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_binary_weights_are_the_region_alignments_to_the_bit(eng, dtype, H, D, r):
    N = 256
    q, k, _ = _feats(3, 100 + r + D, dtype, N, H, D)
    w = _weights(N, [r, r, N], 7 * r + D, 255, 255)
    ia, ib = _idx(0, 1, 2), _idx(1, 2, 0)
    want = eng.pair_align_regions(q, k, w != 0, ia, ib, H, 16, return_attention=True, return_status=True)
    bq, bk = _poison((q, k), w)
    got = eng.pair_align_weights(bq, bk, w, ia, ib, H, 16, return_attention=True, return_status=True, return_sums=True)
    for name, a, b in zip(("match", "weight", "expect", "attn", "status"), got, want):
        assert torch.equal(a, b), name
    assert got[5].tolist() == [255 * r, 255 * r, 255 * N] and got[4].tolist() == [0, 0, 0]


# ---- 2. general bytes by _align64's rules ----------------------------------------------------------------------------------------------
def _check64(eng, q, k, w, pairs, H, label):
    N = q.shape[2]
    gw = _grid_w(N)
    ia, ib = _idx(*(a for a, _ in pairs)), _idx(*(b for _, b in pairs))
    bq, bk = _poison((q, k), w)
    match, weight, expect, attn, st = eng.pair_align_weights(bq, bk, w, ia, ib, H, gw, return_attention=True, return_status=True)
    assert st.tolist() == [0] * len(pairs)
    Pm, bound = soft_align64(q.cpu(), k.cpu(), w.cpu(), pairs, H)
    rows = rows_of(w)
    got = attn.double().cpu()
    worst = 0.0
    for p, (a, b) in enumerate(pairs):
        for d, (x, y) in enumerate(((a, b), (b, a))):
            rq, rk = rows[x], rows[y]
            on = torch.zeros(N, N, dtype=torch.bool)
            on[rq[:, None], rk[None, :]] = True
            g, P, bd = got[p, d], Pm[p, d], bound[p, d]
            assert not g[~on].any()                                                       # zero outside the listed rows and keys
            err = (g - P).abs()[on]
            worst = max(worst, (err / bd[on]).max().item())
            assert (err <= bd[on]).all(), (label, p, d, (err / bd[on]).max().item())
            sums = g[rq].sum(-1)                                                          # probability rows over the listed keys
            assert ((sums - 1).abs() <= (bd[rq].sum(-1) + (len(rk) + 2) * A.U32)).all()
            # off query tokens carry the off values
            offq = torch.ones(N, dtype=torch.bool)
            offq[rq] = False
            m = match[p, d].long().cpu()
            assert (m[offq] == -1).all() and not weight[p, d].cpu()[offq].any() and (expect[p, d].cpu()[offq] == -1).all()
            # match is a near-maximiser among the listed keys (tests/test_gpu_align.py's rule, the bound as the gate)
            sub, sbd, mm = P[rq][:, rk], bd[rq][:, rk], m[rq]
            assert (w.cpu()[y][mm] != 0).all()
            top, jmax = sub.max(-1)
            at, g_at = P[rq, mm], bd[rq, mm]
            g_top = sbd.gather(-1, jmax.unsqueeze(-1)).squeeze(-1)
            tau = 2 * torch.maximum(g_at, g_top) / top
            assert (at >= (1 - tau) * top).all(), ((top - at) / top).max().item()
            wt = weight[p, d].double().cpu()[rq]
            assert ((wt - at).abs() <= g_at).all()
            assert torch.equal(weight[p, d].cpu()[rq], attn[p, d].cpu()[rq, mm])           # the kernel's weight is its own attn at its match
            j = torch.arange(N, dtype=torch.float64)
            coords = torch.stack([torch.div(j, gw, rounding_mode="floor"), j % gw], -1)
            want = g[rq] @ coords
            assert ((expect[p, d].double().cpu()[rq] - want).abs() <= (N / 2 + 2) * A.U32 * want + 1e-30).all()
    print(f"{label} {str(q.dtype)[6:]}: largest attn err / bound {worst:.3f}")
    return worst


@pytest.mark.parametrize("N,H,D", [(256, 8, 160), (256, 4, 40), (196, 8, 72), (64, 4, 32)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("peaked", [False, True])
def test_general_bytes_match_float64(eng, dtype, N, H, D, peaked):
    q, k, _ = _feats(4, 41 + N + D, dtype, N, H, D, logit_scale=4.0 if peaked else 1.0)
    w = _weights(N, _sizes(N), N + D)
    _check64(eng, q, k, w, [(0, 1), (1, 2), (2, 3), (3, 0), (1, 1)], H, f"N={N} H={H} D={D} peaked={peaked}")


@pytest.mark.parametrize("H,D", [(2, 160), (4, 40)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_light_key_with_the_largest_raw_logit(eng, dtype, H, D):
    """tests/test_gpu_soft_regions.py's construction: every image has one key of byte 1 that most queries like best before the bias,
    so the raw maximum the kernels keep is NOT the maximum of the biased logits."""
    N = 256
    q, k, _ = _feats(3, 17 + D, torch.float32, N, H, D, cuda=False)
    g = torch.Generator().manual_seed(D)
    c = torch.randn(H * D, generator=g)
    star = [5, 130, 255]
    q = q + 0.5 * c
    for i, u in enumerate(star):
        k[i, :, u] = (12.0 / D ** 0.5) * c
    q, k = q.to(dtype).contiguous(), k.to(dtype).contiguous()
    w = _weights(N, [N, 200, 129], 3).cpu()
    for i, u in enumerate(star):
        w[i, u] = 1
    for i in range(3):
        rows = torch.nonzero(w[i]).flatten()
        s = heads64(q[(i + 1) % 3], H) @ heads64(k[i], H).index_select(2, rows).transpose(-1, -2)
        assert (rows[s.argmax(-1)] == star[i]).double().mean() > 0.5
    _check64(eng, q.cuda(), k.cuda(), w.cuda(), [(0, 1), (1, 2), (2, 0)], H, f"light key D={D}")


@pytest.mark.parametrize("H,D", [(2, 160), (4, 40), (2, 64)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_heavy_keys_come_last(eng, dtype, H, D):
    """All 256 tokens listed; the first 192 carry byte 1 and the last key tile bytes of 200 .. 255."""
    N = 256
    q, k, _ = _feats(3, 23 + D, dtype, N, H, D)
    w = _weights(N, [N, N, N], 4, 200, 255)
    w[:, :192] = 1
    _check64(eng, q, k, w, [(0, 1), (1, 2), (2, 2)], H, f"heavy last D={D}")


# ---- 3. weights are multiplicities of keys, without an oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("H,D", [(2, 160), (4, 40)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_doubled_key_with_half_the_byte(eng, dtype, H, D):
    """Y: 64 tokens; key u = 9 carries byte 2c.  Y': the same rows with key u a second time at row 64 (bit-identical), both at byte c,
    in a grid of 128 tokens whose other rows have weight 0.  For queries X over the keys Y / Y': the doubled keys' two attn columns
    are equal to the bit and sum to the single key's column, and every other column agrees, within the sum of the two calls' f32
    bounds (tests/_softmap64.py)."""
    n1, u, c = 64, 9, 77
    q, k, _ = _feats(2, 61 + D, dtype, 128, H, D)
    g = torch.Generator().manual_seed(8)
    by = torch.randint(1, 256, (n1,), generator=g)
    by[u] = 2 * c
    wx = torch.randint(1, 256, (128,), generator=g)
    k1, k2 = k.clone(), k.clone()
    k2[1, :, n1] = k2[1, :, u]
    w1 = torch.zeros(2, 128, dtype=torch.uint8)
    w1[0], w1[1, :n1] = wx.to(torch.uint8), by.to(torch.uint8)
    w2 = w1.clone()
    w2[1, u] = w2[1, n1] = c
    ia, ib = _idx(0), _idx(1)
    a = eng.pair_align_weights(q, k1, w1.cuda(), ia, ib, H, 16, return_attention=True)[3][0, 0].double().cpu()
    b = eng.pair_align_weights(q, k2, w2.cuda(), ia, ib, H, 16, return_attention=True)[3][0, 0].double().cpu()
    _, bd1 = soft_align64(q.cpu(), k1.cpu(), w1, [(0, 1)], H)
    _, bd2 = soft_align64(q.cpu(), k2.cpu(), w2, [(0, 1)], H)
    bd1, bd2 = bd1[0, 0], bd2[0, 0]
    assert torch.equal(b[:, u], b[:, n1])                                          # identical rows, identical bytes
    assert ((b[:, u] + b[:, n1] - a[:, u]).abs() <= bd1[:, u] + bd2[:, u] + bd2[:, n1]).all()
    others = [j for j in range(n1) if j != u]
    assert ((b[:, others] - a[:, others]).abs() <= bd1[:, others] + bd2[:, others]).all()
    assert not a[:, n1:].any() and not b[:, n1 + 1:].any()


# ---- 4. ties, invariance, an image without weight -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,H,D,j1,j2", [(torch.bfloat16, 2, 160, 3, 20), (torch.float16, 4, 40, 5, 150), (torch.float32, 2, 72, 37, 250)])
def test_identical_keys_of_equal_weight_tie_to_the_lower_token(eng, dtype, H, D, j1, j2):
    N = 256
    q, k, _ = _feats(3, 5 + D, dtype, N, H, D, cuda=False)
    k[1, :, j1] = (3.0 * q[0, :, 0].float()).to(dtype)
    k[1, :, j2] = k[1, :, j1]
    q[0, :, 1:4] = q[0, :, 0:1]
    w = _weights(N, [200, 180, 90], 12).cpu()
    w[1, j1] = w[1, j2] = 200
    w[0, :4] = 255
    w[1, [j for j in range(N) if j not in (j1, j2)]] = w[1, [j for j in range(N) if j not in (j1, j2)]].clamp(max=200)
    m, wt, ex, at = eng.pair_align_weights(q.cuda(), k.cuda(), w.cuda(), _idx(0, 2), _idx(1, 1), H, 16, return_attention=True)
    for p in range(2):
        assert torch.equal(at[p, 0, :, j1], at[p, 0, :, j2])
        assert not (m[p, 0] == j2).any()
    assert m[0, 0, :4].tolist() == [j1] * 4
    assert wt[0, 0, 0].item() == at[0, 0, 0, j2].item()


@pytest.mark.parametrize("dtype,N,H,D", [(torch.bfloat16, 256, 8, 160), (torch.float32, 144, 2, 72)])
def test_batch_repeat_swap_and_an_image_without_weight(eng, dtype, N, H, D):
    q, k, _ = _feats(4, 81, dtype, N, H, D)
    w = _weights(N, [N // 2, 40, 17, N], 4)
    gw = _grid_w(N)
    ia, ib = _idx(0, 1, 2, 3, 2), _idx(1, 2, 3, 0, 2)
    r1 = eng.pair_align_weights(q, k, w, ia, ib, H, gw, return_attention=True, return_status=True)
    assert r1[4].tolist() == [0] * 5
    assert all(torch.equal(a, b) for a, b in zip(r1, eng.pair_align_weights(q, k, w, ia, ib, H, gw, return_attention=True, return_status=True)))
    one = eng.pair_align_weights(q, k, w, ia[3:4].clone(), ib[3:4].clone(), H, gw, return_attention=True, return_status=True)
    assert all(torch.equal(a[0], b[3]) for a, b in zip(one, r1))
    sw = eng.pair_align_weights(q, k, w, ib, ia, H, gw, return_attention=True)
    assert all(torch.equal(a, b.flip(1)) for a, b in zip(sw, r1[:4]))
    w2 = w.clone()
    w2[2] = 0
    m, wt, ex, at, st, sums = eng.pair_align_weights(q, k, w2, ia, ib, H, gw, return_attention=True, return_status=True, return_sums=True)
    assert st.tolist() == [0, 2, 2, 0, 2] and sums.tolist() == w2.long().sum(1).tolist()
    bad = [1, 2, 4]
    assert (m[bad] == -1).all() and not wt[bad].any() and (ex[bad] == -1).all() and not at[bad].any()
    for got, want in zip((m, wt, ex, at), r1):
        assert torch.equal(got[[0, 3]], want[[0, 3]])
