"""The engine batch every batched call site picks when the caller names none (pairs on 1 and 2 streams, triplets, maps, score
matrix, sweep pairs / triplets at 1 and at 7 taps), for the three scorer kinds, with and without a prompt per row, at three (free
HBM, rows) settings: plenty of memory, memory that forces halvings, fewer rows than the optimum.  Stub engines with the methods
of the real ones (the DiT engine bounds a sweep only) and a workspace linear in the image count; the forward is replaced by a stop
that records the size of the call's first engine batch.  No GPU.

EXPECTED was recorded by running this file's ``_table`` on the commit before the scorers got ``Scorer.auto_rows`` (three
separate sizing functions then); it is a record, not something to regenerate from the code under test.  A changed entry is a
changed chunk size, that is a speed change."""
import pytest
import torch

from diffsim_amd import config as C, harness, maps, retrieval, sweep

GIB = 1 << 30
SETTINGS = {"plenty": (10000 * GIB, 1000), "two_halvings": (80 * GIB, 1000), "few_rows": (10000 * GIB, 5)}


class _Stop(Exception):
    pass


class DiTStubEngine:
    """As DiTEngine: bounds for a sweep only, no context tables."""
    heads, tokens, head_dim = 8, 64, 40

    def max_images_taps(self, taps, upper=4096):
        return 100 if len(taps) == 1 else 60

    def taps_workspace_bytes(self, n, taps):
        return n * (GIB + len(taps) * GIB // 8)


class StubEngine(DiTStubEngine):
    """As UNetEngine; the workspace is `gib` GiB per image, half as much again with a context table."""

    def __init__(self, gib):
        self.gib = gib

    def max_images(self, upper=4096, n_ctx=1):
        return 200 if n_ctx == 1 else 90

    def max_images_taps(self, taps, upper=4096, n_ctx=1):
        return (100 if len(taps) == 1 else 60) - (10 if n_ctx > 1 else 0)

    def workspace_bytes(self, n, n_ctx=1):
        return n * self.gib * GIB * (2 if n_ctx == 1 else 3) // 2

    def taps_workspace_bytes(self, n, taps, n_ctx=1):
        return n * self.gib * (GIB + len(taps) * GIB // 8) * (2 if n_ctx == 1 else 3) // 2

    def tap_shape(self, block, layer):
        return self.tokens, self.heads, self.head_dim

    def set_sample_size(self, side):
        pass


def make(kind):
    from diffsim_amd.diffsim import DiffSim
    from diffsim_amd.diffsim_dit import diffsim_DiT
    from diffsim_amd.diffsim_xl import diffsim_xl
    eng = {"sd15": StubEngine(1), "xl": StubEngine(6), "dit": DiTStubEngine()}[kind]     # (1024-px images: a larger arena each)
    if kind == "sd15":
        s = DiffSim(torch.float32, device="cpu", unet_config=C.TINY, state_dict={})
        flags, taps7 = ("up_blocks", 0), [(b, l) for b in ("down_blocks", "up_blocks") for l in range(3)] + [("mid_blocks", 0)]
        s._base = eng
    elif kind == "xl":
        s = diffsim_xl(torch.float32, "cpu", unet_config=C.SDXL_TINY, state_dict={}, encode_prompt=lambda p: (torch.zeros(1), torch.zeros(1)))
        flags, taps7 = ("up_blocks", [0, 0, 0]), [("up_blocks", [0, 0, t]) for t in range(7)]
        s._base = eng
    else:
        s = diffsim_DiT(128, 600, "cpu", dit_config=C.DIT_TINY, state_dict={}, torch_dtype=torch.float32)
        flags, taps7 = ("none", [0]), list(range(7))
        s._engine = eng
    s.engine = lambda *a: eng
    seen = []

    def stop(lat, *a, **k):
        seen.append(lat.shape[0])
        raise _Stop
    s.features = s.features_taps = stop
    return s, eng, flags, taps7, seen


def first_batch(seen, fn, per_row):
    del seen[:]
    with pytest.raises(_Stop):
        fn()
    assert seen[0] % per_row == 0 or per_row == 1
    return seen[0] // per_row


def _table(monkeypatch):
    out = {}
    for kind in ("sd15", "xl", "dit"):
        for per_row in (False, True):
            for name, (free, n) in SETTINGS.items():
                monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev=None, free=free: (free, 2 * free))
                s, eng, (blk, lay), taps7, seen = make(kind)
                lat, nz = torch.zeros(n, 4, 8, 8), torch.zeros(1, 4, 8, 8)
                if kind == "xl":                    # one prompt per call: a list may only repeat it
                    prompt = ["a"] * n if per_row else "a"
                else:
                    prompt = [("a", "b")[i % 2] for i in range(n)] if per_row else "a"
                if kind == "sd15":
                    row = [s.auto_batch_pairs(eng, n, 1), s.auto_batch_pairs(eng, n, 2)]
                elif kind == "xl":                  # (one stream, and the signature's 8 pairs)
                    row = [first_batch(seen, lambda: s.score_latent_pairs(lat, lat, nz, nz, None, None, blk, lay, 600), 2)] * 2
                else:                               # (one stream, and the signature's 32 pairs)
                    row = [first_batch(seen, lambda: s.score_latent_pairs(lat, lat, nz, nz, 0, 600), 2)] * 2
                row.append(first_batch(seen, lambda: harness.score_latent_triplets(s, lat, lat, lat, nz, nz, prompt, blk, lay, 600), 3))
                row.append(first_batch(seen, lambda: maps.score_latent_pair_maps(s, lat, lat, nz, nz, "a", blk, lay, 600), 2))
                row.append(first_batch(seen, lambda: retrieval.score_latent_matrix(s, lat, lat, nz, nz, "a", blk, lay, 600), 1))
                for taps in ([taps7[0]], taps7):
                    row.append(first_batch(seen, lambda: sweep.score_latent_pairs_taps(s, lat, lat, nz, nz, prompt, taps, 600), 2))
                    row.append(first_batch(seen, lambda: sweep._score_chunks_taps(s, lat, lat, lat, nz, nz, prompt, taps, 600, "cosine",
                                                                                  None), 3))
                out[(kind, per_row, name)] = tuple(row)
    return out


# (kind, a prompt per row, setting): pairs on 1 stream, pairs on 2 streams, triplets, maps (pairs), matrix (images), then sweep
# pairs and sweep triplets at 1 tap and at 7 taps
EXPECTED = {
    ('sd15', False, 'plenty'): (64, 64, 42, 64, 126, 50, 33, 30, 20),
    ('sd15', False, 'two_halvings'): (16, 8, 11, 16, 33, 13, 9, 8, 5),
    ('sd15', False, 'few_rows'): (5, 5, 5, 5, 5, 5, 5, 5, 5),
    ('sd15', True, 'plenty'): (64, 64, 30, 64, 126, 45, 30, 25, 16),
    ('sd15', True, 'two_halvings'): (16, 8, 8, 16, 33, 6, 4, 7, 4),
    ('sd15', True, 'few_rows'): (5, 5, 5, 5, 5, 5, 5, 5, 5),
    ('xl', False, 'plenty'): (8, 8, 5, 7, 15, 8, 5, 8, 5),
    ('xl', False, 'two_halvings'): (8, 8, 2, 3, 6, 2, 1, 1, 1),
    ('xl', False, 'few_rows'): (5, 5, 5, 5, 5, 5, 5, 5, 5),
    ('xl', True, 'plenty'): (8, 8, 5, 7, 15, 8, 5, 8, 5),
    ('xl', True, 'two_halvings'): (8, 8, 2, 3, 6, 2, 1, 1, 1),
    ('xl', True, 'few_rows'): (5, 5, 5, 5, 5, 5, 5, 5, 5),
    ('dit', False, 'plenty'): (32, 32, 42, 63, 126, 50, 33, 30, 20),
    ('dit', False, 'two_halvings'): (32, 32, 42, 63, 126, 13, 9, 8, 5),
    ('dit', False, 'few_rows'): (5, 5, 5, 5, 5, 5, 5, 5, 5),
    ('dit', True, 'plenty'): (32, 32, 42, 63, 126, 50, 33, 30, 20),
    ('dit', True, 'two_halvings'): (32, 32, 42, 63, 126, 13, 9, 8, 5),
    ('dit', True, 'few_rows'): (5, 5, 5, 5, 5, 5, 5, 5, 5),
}


def test_every_call_site_picks_the_recorded_engine_batch(monkeypatch):
    got = _table(monkeypatch)
    assert got[("dit", False, "plenty")][3] == 63 and got[("xl", False, "plenty")][3] == 7       # maps: 3 * triplets // 2
    assert got == EXPECTED
