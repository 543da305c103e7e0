"""Host side of many prompts per U-Net forward: the context-table builder, the engine's argument checks and the scorers' rule
for which kinds batch across prompts.  No GPU."""
import pytest
import torch

from diffsim_amd import _lib, config as C, synth as S


def _scorer(encoded):
    from diffsim_amd.diffsim import DiffSim
    ctx = {p: S.make_context(C.TINY, seed=i) for i, p in enumerate(["a", "b", "c"])}

    def encode(p):
        encoded.append(p)
        return ctx[p]
    return DiffSim(torch.float32, device="cpu", unet_config=C.TINY, state_dict={}, encode_prompt=encode), ctx


def test_table_in_order_of_first_appearance_each_prompt_encoded_once():
    from diffsim_amd.diffsim import PromptTable
    enc = []
    ds, ctx = _scorer(enc)
    t = ds.prompt_table(["b", "a", "b", "c", "a", "b"])
    assert isinstance(t, PromptTable)
    assert t.index == [0, 1, 0, 2, 1, 0]
    assert t.table.shape == (3, 2, C.TINY.ctx_len, C.TINY.cross_attention_dim) and t.table.dtype == torch.float32
    for row, p in enumerate(["b", "a", "c"]):
        assert torch.equal(t.table[row], ctx[p])
    assert enc == ["b", "a", "c"]
    ds.prompt_table(["c", "a"])
    assert enc == ["b", "a", "c"]                   # the context() cache: no prompt twice


def test_table_of_tensor_and_string_prompts():
    enc = []
    ds, ctx = _scorer(enc)
    x, y = S.make_context(C.TINY, seed=40), S.make_context(C.TINY, seed=41)
    t = ds.prompt_table([x, "a", y, x, "a"])
    assert t.index == [0, 1, 2, 0, 1]
    assert torch.equal(t.table[0], x) and torch.equal(t.table[1], ctx["a"]) and torch.equal(t.table[2], y)
    assert enc == ["a"]


def test_one_prompt_collapses_to_the_one_prompt_call():
    from diffsim_amd.diffsim import row_prompts
    enc = []
    ds, ctx = _scorer(enc)
    one = ds.prompt_table(["a"] * 4)
    assert isinstance(one, torch.Tensor) and torch.equal(one, ctx["a"])
    x = S.make_context(C.TINY, seed=40)
    assert torch.equal(ds.prompt_table([x, x]), x)
    c, idx = ds._contexts(["b", "b", "b"], 3)
    assert idx is None and torch.equal(c, ctx["b"])
    c, idx = ds._contexts("b", 3)
    assert idx is None and torch.equal(c, ctx["b"])
    c, idx = ds._contexts(["b", "c", "b"], 3)
    assert idx == [0, 1, 0] and c.shape[0] == 2
    with pytest.raises(ValueError):
        ds._contexts(["b", "c"], 3)                 # one prompt per image
    # rows of a chunk, image by image; one prompt of the call stays as it is
    assert row_prompts(["p", "q", "r"], 1, 3, 3) == ["q"] * 3 + ["r"] * 3
    assert row_prompts("p", 1, 3, 2) == "p"
    assert row_prompts(x, 0, 1, 2) is x


def test_engine_host_checks():
    from diffsim_amd.engine import check_ctx_table
    cfg = C.TINY
    L, Dc = cfg.ctx_len, cfg.cross_attention_dim
    table = torch.zeros(3, 2, L, Dc)
    n_ctx, idx = check_ctx_table(cfg, table, [2, 0, 1, 1], 4)
    assert n_ctx == 3 and idx.dtype == torch.int32 and idx.tolist() == [2, 0, 1, 1] and not idx.is_cuda
    assert check_ctx_table(cfg, torch.zeros(2, L, Dc), None, 4) == (1, None)
    assert check_ctx_table(cfg, torch.zeros(1, 2, L, Dc), [0, 0], 2) == (1, None)      # a table of one row: the one-prompt call
    for bad in ([3, 0, 1, 1], [0, -1, 1, 1]):
        with pytest.raises(_lib.DsimError, match="range|lie in"):
            check_ctx_table(cfg, table, bad, 4)                    # out of range
    with pytest.raises(_lib.DsimError, match="entries"):
        check_ctx_table(cfg, table, [0, 1, 2], 4)                  # index length != images
    with pytest.raises(_lib.DsimError, match="ctx_index"):
        check_ctx_table(cfg, table, None, 4)                       # a table without an index
    with pytest.raises(_lib.DsimError):
        check_ctx_table(cfg, torch.zeros(3, 2, L + 1, Dc), [0, 1, 2, 0], 4)       # wrong table shape
    with pytest.raises(_lib.DsimError):
        check_ctx_table(cfg, torch.zeros(3, 1, L, Dc), [0, 1, 2, 0], 4)
    with pytest.raises(_lib.DsimError):
        check_ctx_table(cfg, torch.zeros(2, L, Dc, 1, 1), [0, 1, 2, 0], 4)
    with pytest.raises(_lib.DsimError, match="integers"):
        check_ctx_table(cfg, table, torch.tensor([0.0, 1.0, 2.0, 0.0]), 4)
    with pytest.raises(_lib.DsimError, match="range|lie in"):
        check_ctx_table(cfg, torch.zeros(2, L, Dc), [0, 1], 2)      # (2, L, Dc): only row 0 exists


def test_scorers_decide_which_kinds_batch_across_prompts():
    from diffsim_amd.diffsim_dit import diffsim_DiT
    from diffsim_amd.diffsim_xl import diffsim_xl
    enc = []
    sd, _ = _scorer(enc)
    assert sd.mixes_prompts and sd.group_key("a") is None and sd.group_key("b") is None
    assert sd.group_prompt(["a", "b", "a"]) == ["a", "b", "a"]
    assert sd.group_prompt(["a", "a"]) == "a"
    assert sd.chunk_prompt(["a", "b", "c"], 1, 3, 3) == ["b"] * 3 + ["c"] * 3
    assert sd.prompt_rows(["a", "b"], 2) == ["a", "b"]
    with pytest.raises(ValueError):
        sd.prompt_rows(["a", "b"], 3)
    xl = diffsim_xl(torch.float32, "cpu", unet_config=C.SDXL_TINY, state_dict={})
    assert not xl.mixes_prompts and xl.group_key("a") == "a" and xl.group_key("b") == "b"
    assert xl.group_prompt(["a", "a"]) == "a"
    assert xl.chunk_prompt("a", 0, 2, 3) == "a"
    assert xl.prompt_rows(["a", "a"], 2) == "a"
    with pytest.raises(ValueError, match="one prompt"):
        xl.prompt_rows(["a", "b"], 2)
    dit = diffsim_DiT(128, 600, "cpu", dit_config=C.DIT_TINY, state_dict={}, torch_dtype=torch.float32)
    assert dit.mixes_prompts and dit.group_key("a") is None and dit.group_key("b") is None
