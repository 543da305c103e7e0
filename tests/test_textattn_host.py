"""Text attention maps and text-guided regions, the parts that need no GPU: the C ABI's declarations and refusals, the prompt's token
weights, the command line, tests/_textattn64.py against a hand-written softmax, and the two conditions on the test inputs that
tests/test_gpu_textattn.py relies on (the near-threshold cap and the planted family's margins)."""
import ctypes
import math
import os
import re

import pytest
import torch

from tests import _textattn64 as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_lib_and_library_agree_on_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "diffsim_amd.h")).read()
    assert re.search(r"#define\s+DSIM_ABI_VERSION\s+7\b", hdr)             # additive: the version stays
    from diffsim_amd import _lib
    assert _lib.ABI_VERSION == 7
    L = _lib.lib()
    assert L.dsim_version() == 7
    for name, nargs in (("dsim_unet_text_workspace_bytes", 3), ("dsim_unet_qkv_text", 17), ("dsim_text_attention_workspace_bytes", 3),
                        ("dsim_text_attention", 22)):
        assert len(_lib.SYMBOLS[name][1]) == nargs, name
        decl = re.search(r"(?:int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == nargs, name
        assert getattr(L, name) is not None
    assert "argprocess.py:17" in hdr


def test_refusals_come_before_any_launch():
    """Every refusal of dsim_text_attention is decided on the host before anything is enqueued, so it is checked without a GPU (the
    pointers are never read)."""
    from diffsim_amd import _lib
    L = _lib.lib()
    n, N, H, D, Lk = 3, 49, 2, 16, 13
    wsb = L.dsim_text_attention_workspace_bytes
    need = int(wsb(n, N, Lk))
    assert need == n * N * 4 + 256
    for args in ((0, N, Lk), (n, 0, Lk), (n, N, 0), (n, N, 129), (65536, N, Lk)):
        assert wsb(*args) == 0, args
    assert wsb(65535, N, 128) > 0
    fake = ctypes.c_void_p(0x10000)

    def go(xq=fake, xk=fake, ldq=H * D, ldk=2 * H * D, n=n, n_kv=2 * n, H=H, N=N, Lk=Lk, D=D, dtype=_lib.DSIM_BF16, w=fake, n_w=1, thr=1.0,
           sal=fake, mask=fake, ws=need):
        rc = L.dsim_text_attention(xq, ldq, xk, ldk, n, n_kv, H, N, Lk, D, dtype, w, n_w, thr, None, sal, mask, None, None, fake, ws, None)
        return L.dsim_strerror(rc).lower()

    assert b"workspace" in go(ws=need - 257)          # (the query adds 256 bytes of alignment slack; the pointer here is aligned)
    assert b"workspace" in go(ws=0)
    for kw in (dict(dtype=9), dict(dtype=-1), dict(D=24), dict(D=0), dict(Lk=0), dict(Lk=129), dict(n_kv=3), dict(n_kv=4), dict(n_kv=0),
               dict(n_w=2), dict(n_w=0), dict(w=None), dict(thr=-0.5), dict(thr=float("nan")), dict(thr=float("inf")), dict(n=0),
               dict(H=0), dict(N=0), dict(xq=None), dict(xk=None), dict(ldq=H * D - 8), dict(ldk=H * D + 2),
               dict(xq=ctypes.c_void_p(0x10008))):
        for dtype in ((_lib.DSIM_BF16, _lib.DSIM_F16, _lib.DSIM_F32) if "dtype" not in kw else (kw["dtype"],)):
            assert b"invalid" in go(**{**kw, "dtype": dtype}), (kw, dtype)
    # without saliency or a region the weights may be NULL and n_w anything: the refusal is then the workspace's
    assert b"workspace" in go(w=None, n_w=7, sal=None, mask=None, ws=0)


# ---- the prompt's token weights -------------------------------------------------------------------------------------------------------
_Words = X.WordTokenizer


def test_prompt_token_weights():
    from diffsim_amd.textattn import prompt_token_weights as ptw
    tok = _Words()
    assert ptw(tok, "The photo of a cat").tolist() == [0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0]                  # the content span
    assert ptw(tok, "The photo of a cat", ["cat"]).tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert ptw(tok, "a red snowboard here", ["snowboard"]).tolist() == [0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0]   # a word of two tokens
    assert ptw(tok, "a red snowboard here", ["red snowboard", "a"]).tolist() == [0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert ptw(tok, "cat and cat", ["cat"]).tolist() == [0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0]                 # every occurrence
    assert ptw(tok, "", None).tolist() == [0] * 12                                                           # nothing between BOS and EOS
    with pytest.raises(ValueError, match="dog"):
        ptw(tok, "The photo of a cat", ["cat", "dog"])
    with pytest.raises(ValueError, match="board"):
        ptw(tok, "a snow scene", ["snowboard"])                                                              # half a run is no hit
    with pytest.raises(ValueError, match="weights"):
        ptw(tok, torch.zeros(2, 12, 8))                                                                      # a context tensor
    with pytest.raises(ValueError, match="tokenizer"):
        ptw(None, "a cat")
    long = ptw(_Words(6), "one two three four five six seven")                                               # truncated before its EOS
    assert long.tolist() == [0, 1, 1, 1, 1, 0]


def test_text_guide_binds_one_weight_row_per_row():
    from diffsim_amd.textattn import TextGuide

    class S:
        device, tokenize = torch.device("cpu"), _Words()
    w = TextGuide(["cat"]).bind(S, "a cat", 3)
    assert w.shape == (12,) and w.tolist()[:4] == [0, 0, 1, 0]
    w = TextGuide().bind(S, ["a cat", "the big dog", "a cat"], 3)
    assert w.shape == (3, 12) and w.sum(1).tolist() == [2, 3, 2]
    with pytest.raises(ValueError):
        TextGuide().bind(S, ["a cat", "a dog"], 3)
    given = torch.arange(12.0)
    assert torch.equal(TextGuide(weights=given).bind(S, torch.zeros(2, 12, 8), 3), given)                    # a context tensor with weights
    with pytest.raises(ValueError, match="weights"):
        TextGuide().bind(S, torch.zeros(2, 12, 8), 3)
    with pytest.raises(ValueError, match="weights"):
        TextGuide().bind(S, (torch.zeros(2, 12, 8), torch.zeros(2, 4)), 3)                                   # SDXL's (context, pooled)
    for thr in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            TextGuide(rel_threshold=thr)


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_text_attn_is_for_the_one_tap_cute_and_nights_runs(capsys):
    from diffsim_amd.cli import arg_parse
    a = arg_parse(["--dataset", "cute", "--text_attn"])
    assert a.text_attn == [] and a.use_text_attn is True and a.text_threshold == 1.0
    b = arg_parse(["--dataset", "nights", "--text_attn", "cat", "dog", "--text_threshold", "0.5", "--metric", "diffsim_xl"])
    assert b.text_attn == ["cat", "dog"] and b.text_threshold == 0.5 and b.use_text_attn is True
    c = arg_parse(["--use_text_attn"])                                       # accepted and without effect, as before
    assert c.use_text_attn is True and c.text_attn is None
    assert arg_parse([]).use_text_attn is False and arg_parse([]).text_attn is None
    for extra in (["--dataset", "sref"], ["--dataset", "retrieval"], ["--dataset", "cute", "--taps", "up_blocks:0"],
                  ["--dataset", "cute", "--mask_path", "m"], ["--metric", "dit"], ["--text_threshold", "-1"],
                  ["--text_threshold", "nan"]):
        with pytest.raises(SystemExit) as e:
            arg_parse(extra + ["--text_attn"])
        assert e.value.code == 2, extra
        assert "--text_" in capsys.readouterr().err


def test_dit_has_no_text_regions():
    from diffsim_amd.diffsim_dit import diffsim_DiT
    for name in ("text_region_score", "text_attention_map"):
        with pytest.raises(NotImplementedError, match="text"):
            getattr(diffsim_DiT, name)(object())


# ---- tests/_textattn64.py -------------------------------------------------------------------------------------------------------------
def test_helper_against_a_hand_written_two_head_softmax():
    """N = 2 tokens, H = 2 heads of D = 2, L = 3 keys, worked through with math.exp."""
    xq = torch.zeros(1, 2, 2, 4)
    xq[0, 1] = torch.tensor([[1.0, 0.0, 0.0, 2.0], [0.0, 1.0, 1.0, 1.0]])
    xq[0, 0] = 9.0                                                           # the unconditional half is never read
    xkv = torch.zeros(2, 3, 8)
    xkv[1, :, :4] = torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 2.0, 1.0, 0.0], [1.0, 1.0, 0.0, 1.0]])
    xkv[0] = 7.0
    xkv[1, :, 4:] = 5.0                                                      # nor is V
    T, bound = X.attn64(xq, xkv, 2)
    r2 = math.sqrt(2.0)

    def sm(ts):
        e = [math.exp(t / r2) for t in ts]
        return [v / sum(e) for v in e]
    # token 0: head 0 q = (1, 0): logits 1, 0, 1; head 1 q = (0, 2): logits 0, 0, 2
    # token 1: head 0 q = (0, 1): logits 0, 2, 1; head 1 q = (1, 1): logits 0, 1, 1
    want = [[(a + b) / 2 for a, b in zip(sm([1, 0, 1]), sm([0, 0, 2]))], [(a + b) / 2 for a, b in zip(sm([0, 2, 1]), sm([0, 1, 1]))]]
    assert torch.allclose(T[0], torch.tensor(want, dtype=torch.float64), rtol=0, atol=1e-15)
    assert (bound > 0).all() and (bound < 1e-5).all()
    w = torch.tensor([0.0, 2.0, 1.0])
    s = X.saliency64(T, w)
    assert abs(s[0, 0].item() - (2 * want[0][1] + want[0][2])) < 1e-15
    on, cnt, m = X.region64(s)
    assert abs(m[0].item() - s[0].mean().item()) < 1e-18 and cnt.tolist() == [1]
    assert X.region64(s, 0.0)[1].tolist() == [2] and X.region64(s, 50.0)[1].tolist() == [2]                  # every token; the fallback
    nan = s.clone()
    nan[0, 0] = float("nan")
    assert X.region64(nan)[0].all()                                                                          # non-finite: the whole image
    # one shared [uncond, cond] context == a context per batch element
    assert torch.equal(X.attn64(xq.repeat(2, 1, 1, 1), xkv, 2, False)[0][1], T[0])


# ---- the conditions on the inputs of tests/test_gpu_textattn.py -----------------------------------------------------------------------
@pytest.mark.parametrize("family", list(X.FAMILIES))
@pytest.mark.parametrize("N,H,D,L", [s for s in X.SHAPES if s[3] > 1], ids=lambda v: str(v))
def test_near_threshold_cap(N, H, D, L, family):
    """The mask check excludes the tokens inside the band around the threshold; the band may hold at most BAND_SHARE of a case's
    tokens, in every dtype of the case -- a condition on the inputs, checked here in float64 with the gates the GPU test uses.
    (L = 1 has a constant saliency: every token sits on the threshold; the GPU test checks that case exactly instead.)"""
    for dtype in X.SHAPES[(N, H, D, L)]:
        xq, xkv = X.operands(X.N_IMAGES, 7 + N + D + L, dtype, N, H, D, L, X.FAMILIES[family])
        T, bound = X.attn64(xq, xkv, H)
        w = X.weights(L)
        s = X.saliency64(T, w)
        sgate = X.saliency_gate(T, X.attn_gate(T, bound, family), w)
        share = X.band(s, sgate).double().mean(-1)
        on = X.region64(s)[0].double().mean(-1)
        print(f"{str(dtype)[6:]} N={N} H={H} D={D} L={L} {family}: in band {share.max().item():.4f}  on {on.min().item():.3f}-{on.max().item():.3f}")
        assert share.max().item() <= X.BAND_SHARE
        assert 0.05 <= on.min().item() and on.max().item() <= 0.95                # the regions are neither empty nor the whole image


@pytest.mark.parametrize("dtype", X.ALL3, ids=["bfloat16", "float16", "float32"])
@pytest.mark.parametrize("N,H,D,L", X.PLANTED)
def test_planted_margins(N, H, D, L, dtype):
    """min over S of s >= 2 m and max outside S of s <= m / 2 in the reference: the kernel's mask must then be S exactly."""
    xq, xkv, w, S = X.planted(5 + N + L, dtype, N, H, D, L, X.planted_gain(D))
    T, bound = X.attn64(xq, xkv, H)
    s = X.saliency64(T, w)[0]
    m = s.mean()
    assert 0 < int(S.sum()) < N and abs(int(S.sum()) - N / 4) <= 1
    assert s[S].min() >= 2 * m and s[~S].max() <= m / 2, (s[S].min().item(), s[~S].max().item(), m.item())
    assert torch.equal(X.region64(s[None])[0][0], S)
    # ... and the margins (>= m on S, >= m / 2 off it) are far above what f32 can move: the saliency gate, twice for the mean
    assert 2 * X.saliency_gate(T, bound, w).max() < m / 8
