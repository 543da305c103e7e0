"""Text attention maps and regions on the GPU (csrc/textattn.hip behind dsim_text_attention), through the C ABI, against the float64
restatement, bound and gates of tests/_textattn64.py.

Inputs: 3 images of seeded randn operands, a context per batch element, q scaled by 1 (ordinary) and by 3 (scaled); weights 1 on
tokens 5-7 (1-3 when L = 13, token 0 when L = 1).  Each case's operands, float64 reference and kernel outputs are computed once
(_case) and shared by the checks.  Every figure is printed before it is asserted."""
import ctypes
import functools

import pytest
import torch

from tests import _textattn64 as X

pytestmark = pytest.mark.gpu

CASES = [(N, H, D, L, dt) for (N, H, D, L), dts in X.SHAPES.items() for dt in dts]
IDS = [f"{N}-{H}-{D}-{L}-{str(dt)[6:]}" for N, H, D, L, dt in CASES]
SMALL = [c for c in CASES if c[0] <= 256 and c[2] in (16, 40, 160, 32)]
SMALL_IDS = [f"{N}-{H}-{D}-{L}-{str(dt)[6:]}" for N, H, D, L, dt in SMALL]
NAMES = ("attn", "saliency", "mask", "counts", "status")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def call(xq, xkv, H, w=None, thr=1.0, want=NAMES, ws_bytes=None, **over):
    """dsim_text_attention through the C ABI on device tensors; (rc, {name: tensor}) with the outputs named in want, each pre-filled
    with a sentinel.  over: raw argument overrides (ldq, ldk, n_kv, L, D, dtype, n_w)."""
    from diffsim_amd import _lib
    from diffsim_amd.engine import _TORCH2DSIM
    Lb = _lib.lib()
    n, _, N, HD = xq.shape
    n_kv, L = xkv.shape[0], xkv.shape[1]
    o = {"attn": torch.full((n, N, L), -7.0, device="cuda"),
         "saliency": torch.full((n, N), -7.0, device="cuda"),
         "mask": torch.full((n, N), 7, dtype=torch.uint8, device="cuda"),
         "counts": torch.full((n,), -7, dtype=torch.int32, device="cuda"),
         "status": torch.full((n,), -7, dtype=torch.int32, device="cuda")}
    o = {name: t for name, t in o.items() if name in want}
    need = int(Lb.dsim_text_attention_workspace_bytes(n, N, L))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    n_w = 1 if w is None or w.ndim == 1 else w.shape[0]
    a = dict(ldq=HD, ldk=2 * HD, n_kv=n_kv, H=H, L=L, D=HD // max(H, 1), dtype=_TORCH2DSIM[xq.dtype], n_w=n_w)
    a.update(over)
    rc = Lb.dsim_text_attention(_p(xq), a["ldq"], _p(xkv), a["ldk"], n, a["n_kv"], a["H"], N, a["L"], a["D"], a["dtype"], _p(w), a["n_w"],
                                float(thr), _p(o.get("attn")), _p(o.get("saliency")), _p(o.get("mask")), _p(o.get("counts")),
                                _p(o.get("status")), _p(ws), need if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    return rc, o


@functools.lru_cache(maxsize=None)
def _case(N, H, D, L, dtype, family):
    """(xq, xkv, w on the device, T64, gate, s64, sgate, kernel outputs on the CPU) of one case, computed once"""
    xq, xkv = X.operands(X.N_IMAGES, 7 + N + D + L, dtype, N, H, D, L, X.FAMILIES[family])
    w = X.weights(L)
    T, bound = X.attn64(xq, xkv, H)
    gate = X.attn_gate(T, bound, family)
    s = X.saliency64(T, w)
    sgate = X.saliency_gate(T, gate, w)
    xqd, xkd, wd = xq.cuda(), xkv.cuda(), w.cuda()
    rc, o = call(xqd, xkd, H, wd)
    assert rc == 0
    return xqd, xkd, wd, T, gate, s, sgate, {name: t.cpu() for name, t in o.items()}


@pytest.mark.parametrize("family", list(X.FAMILIES))
@pytest.mark.parametrize("N,H,D,L,dtype", CASES, ids=IDS)
def test_attn_saliency_and_mask_match_float64(N, H, D, L, dtype, family):
    _, _, _, T, gate, s, sgate, o = _case(N, H, D, L, dtype, family)
    assert o["status"].tolist() == [0] * X.N_IMAGES
    attn = o["attn"].double()
    ratio = ((attn - T).abs() / gate).max().item()
    rows = (attn.sum(-1) - 1).abs().max().item()
    sratio = ((o["saliency"].double() - s).abs() / sgate).max().item()
    want, counts, _ = X.region64(s)
    near = X.band(s, sgate)
    share = near.double().mean(-1).max().item()
    got = o["mask"].bool()
    print(f"{str(dtype)[6:]} N={N} H={H} D={D} L={L} {family}: attn err/gate {ratio:.3f}  row sum err {rows:.2e}  saliency err/gate "
          f"{sratio:.3f}  in band {share:.4f}  on {want.double().mean().item():.3f}  mask flips outside band "
          f"{int(((got != want) & ~near).sum())}")
    assert ratio <= 1.0
    assert rows <= L * 2.0 ** -23
    assert sratio <= 1.0
    assert set(o["mask"].unique().tolist()) <= {0, 1}
    assert torch.equal(o["counts"].long(), got.sum(-1))
    if L == 1:
        # T == 1 exactly: the saliency is the weight, the mean is the weight, every token is on its threshold and on
        assert (o["attn"] == 1.0).all() and (o["saliency"] == 1.0).all() and got.all()
        return
    assert share <= X.BAND_SHARE
    assert torch.equal(got[~near], want[~near])


@pytest.mark.parametrize("dtype", X.ALL3, ids=["bfloat16", "float16", "float32"])
@pytest.mark.parametrize("N,H,D,L", X.PLANTED)
def test_planted_region_is_recovered_exactly(N, H, D, L, dtype):
    xq, xkv, w, S = X.planted(5 + N + L, dtype, N, H, D, L, X.planted_gain(D))
    rc, o = call(xq.cuda(), xkv.cuda(), H, w.cuda())
    assert rc == 0 and o["status"].tolist() == [0]
    assert torch.equal(o["mask"][0].bool().cpu(), S)
    assert o["counts"].tolist() == [int(S.sum())]


@pytest.mark.parametrize("N,H,D,L,dtype", SMALL, ids=SMALL_IDS)
def test_threshold_edges(N, H, D, L, dtype):
    xqd, xkd, wd, _, _, s, _, first = _case(N, H, D, L, dtype, "ordinary")
    rc, o = call(xqd, xkd, H, wd, thr=0.0)                                      # non-negative weights: s >= 0 = 0 m
    assert rc == 0 and o["mask"].bool().all() and o["counts"].tolist() == [N] * X.N_IMAGES
    assert torch.equal(o["saliency"].cpu(), first["saliency"])
    top = float((s.max(-1).values / s.mean(-1)).max())
    rc, o = call(xqd, xkd, H, wd, thr=2.0 * top + 1.0)                          # above every token: the all-on fallback
    assert rc == 0 and o["mask"].bool().all() and o["counts"].tolist() == [N] * X.N_IMAGES


@pytest.mark.parametrize("N,H,D,L,dtype", SMALL, ids=SMALL_IDS)
def test_deterministic_batch_invariant_and_output_independent(N, H, D, L, dtype):
    xqd, xkd, wd, _, _, _, _, first = _case(N, H, D, L, dtype, "ordinary")
    n = X.N_IMAGES
    rc, again = call(xqd, xkd, H, wd)
    assert rc == 0 and all(torch.equal(again[k].cpu(), first[k]) for k in NAMES)                     # repeat calls
    # image 1 alone == image 1 inside a batch of 5 (at another position)
    xq5 = torch.cat([xqd[2:3], xqd[0:1], xqd[0:1], xqd[1:2], xqd[2:3]]).contiguous()
    xk5 = torch.cat([xkd[4:6], xkd[0:2], xkd[0:2], xkd[2:4], xkd[4:6]]).contiguous()
    rc, five = call(xq5, xk5, H, wd)
    rc1, one = call(xqd[1:2].contiguous(), xkd[2:4].contiguous(), H, wd)
    assert rc == 0 and rc1 == 0
    for k in NAMES:
        assert torch.equal(five[k][3].cpu(), first[k][1]) and torch.equal(one[k][0].cpu(), first[k][1]), k
    for k in NAMES:                                                                                  # any subset may be NULL
        rc, only = call(xqd, xkd, H, wd, want=(k,))
        assert rc == 0 and torch.equal(only[k].cpu(), first[k]), k
    rc, lean = call(xqd, xkd, H, None, want=("attn", "status"))                                      # no weights: attn alone
    assert rc == 0 and torch.equal(lean["attn"].cpu(), first["attn"])
    rc, none = call(xqd, xkd, H, wd, want=())
    assert rc == 0
    # one shared [uncond, cond] context == the same context repeated per batch element
    shared = xkd[0:2].contiguous()
    rc, a = call(xqd, shared, H, wd)
    rc2, b = call(xqd, shared.repeat(n, 1, 1).contiguous(), H, wd)
    assert rc == 0 and rc2 == 0 and all(torch.equal(a[k], b[k]) for k in NAMES)
    # shared weights == per-image copies
    rc, c = call(xqd, xkd, H, wd[None].repeat(n, 1).contiguous())
    assert rc == 0 and all(torch.equal(c[k].cpu(), first[k]) for k in NAMES)
    # per-image weights are per image: image 1 with other weights moves image 1 alone
    w2 = wd[None].repeat(n, 1).contiguous()
    w2[1] = torch.roll(w2[1], 1)
    rc, d = call(xqd, xkd, H, w2)
    assert rc == 0 and torch.equal(d["saliency"][[0, 2]].cpu(), first["saliency"][[0, 2]])
    assert L == 1 or not torch.equal(d["saliency"][1].cpu(), first["saliency"][1])


@pytest.mark.parametrize("N,H,D,L,dtype", [(81, 4, 40, 77, torch.bfloat16), (49, 2, 16, 13, torch.float32), (70, 1, 32, 128, torch.float16)])
def test_nan_key_flags_exactly_the_images_with_that_context(N, H, D, L, dtype):
    xqd, xkd, wd, _, _, _, _, first = _case(N, H, D, L, dtype, "ordinary")
    k2 = xkd.clone()
    k2[3, L // 2, 5] = float("nan")                          # image 1's cond context (row 2 * 1 + 1), a K column
    rc, o = call(xqd, k2, H, wd)
    assert rc == 0 and o["status"].tolist() == [0, 1, 0]
    assert o["mask"][1].bool().all() and o["counts"][1].item() == N              # non-finite saliency: the whole image
    for k in NAMES:
        assert torch.equal(o[k][[0, 2]].cpu(), first[k][[0, 2]]), k
    k3 = xkd.clone()
    k3[2, 0, 0] = float("nan")                               # image 1's uncond context: never read
    k3[3, 0, H * D] = float("nan")                           # ... and a V column of its cond context
    rc, o = call(xqd, k3, H, wd)
    assert rc == 0 and all(torch.equal(o[k].cpu(), first[k]) for k in NAMES)
    shared = xkd[0:2].clone()
    shared[1, 0, 0] = float("nan")                           # one shared context: every image uses it
    rc, o = call(xqd, shared, H, wd)
    assert rc == 0 and o["status"].tolist() == [1, 1, 1] and o["mask"].bool().all()


def test_every_refusal_comes_before_anything_is_enqueued():
    from diffsim_amd import _lib
    N, H, D, L = 49, 2, 16, 13
    xq, xkv = X.operands(3, 1, torch.bfloat16, N, H, D, L)
    xqd, xkd, wd = xq.cuda(), xkv.cuda(), X.weights(L).cuda()
    inv, wsp = -1, -3                                                            # DSIM_ERR_INVALID, DSIM_ERR_WORKSPACE
    bad = [(dict(dtype=9), inv), (dict(D=24), inv), (dict(L=0), inv), (dict(L=129), inv), (dict(n_kv=3), inv), (dict(n_kv=4), inv),
           (dict(n_w=2), inv), (dict(H=0), inv), (dict(ldq=H * D - 8), inv), (dict(ldk=H * D + 4), inv)]
    for over, code in bad:
        over = dict(over)
        rc, o = call(xqd, xkd, over.pop("H", H), wd, **over)
        assert rc == code, (over, rc)
        _untouched(o)
    for thr in (-1.0, float("nan"), float("inf")):
        rc, o = call(xqd, xkd, H, wd, thr=thr)
        assert rc == inv, thr
        _untouched(o)
    for want in (("saliency",), ("mask",), ("counts",)):                         # a NULL weight with saliency or a region asked for
        rc, o = call(xqd, xkd, H, None, want=want)
        assert rc == inv, want
        _untouched(o)
    need = int(_lib.lib().dsim_text_attention_workspace_bytes(3, N, L))
    rc, o = call(xqd, xkd, H, wd, ws_bytes=need - 256 - 1)                       # (the query adds the alignment slack: one byte short of the rest)
    assert rc == wsp
    _untouched(o)
    rc, o = call(xqd, xkd, H, wd, ws_bytes=0)
    assert rc == wsp
    _untouched(o)
    Lb = _lib.lib()
    assert Lb.dsim_text_attention_workspace_bytes(0, N, L) == 0 and Lb.dsim_text_attention_workspace_bytes(3, 0, L) == 0
    assert Lb.dsim_text_attention_workspace_bytes(3, N, 0) == 0 and Lb.dsim_text_attention_workspace_bytes(3, N, 129) == 0
    assert Lb.dsim_text_attention_workspace_bytes(3, N, 128) == 3 * N * 4 + 256


def _untouched(o):
    for name, t in o.items():
        assert (t == (7 if name == "mask" else -7)).all(), name


def test_engine_wrapper_returns_what_the_abi_returns():
    from diffsim_amd import engine
    N, H, D, L = 81, 4, 40, 77
    xqd, xkd, wd, _, _, _, _, first = _case(N, H, D, L, torch.float16, "ordinary")
    out = engine.text_attention(xqd, xkd, H, wd, want=NAMES)
    assert out["mask"].dtype == torch.bool
    assert torch.equal(out["mask"].cpu(), first["mask"].bool())
    assert all(torch.equal(out[k].cpu(), first[k]) for k in ("attn", "saliency", "counts", "status"))
    lean = engine.text_attention(xqd, xkd, H, wd)
    assert sorted(lean) == ["counts", "mask", "saliency"] and torch.equal(lean["mask"], out["mask"])
    with pytest.raises(Exception):
        engine.text_attention(xqd, xkd, H, None)
    with pytest.raises(ValueError):
        engine.text_attention(xqd, xkd, H, wd, want=("nope",))
