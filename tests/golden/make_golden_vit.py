#!/usr/bin/env python3
"""Generate g11_vit_tails.npz by running the REFERENCE's own score tails of the ViT metrics.

Runs only where the reference checkout is (/root/reference); only the data file it writes travels.  metrics/clip_i.py and
metrics/dino.py import third-party packages that may not be installed (fire, megfile, tqdm, torchvision): name-only stubs are registered for them,
as make_golden.py does for the diffusion files.  ``CLIPScore.attention_calc`` (clip_i.py:113-128) and
``Dinov2Score.attention_calc`` (dino.py:120-132) then execute unmodified on seeded q / k / v, followed by the cosine and the mean of
``clip_cross_score`` / ``dino_cross_score`` (clip_i.py:152-159, dino.py:154-161), which are restated here line for line because the
methods themselves need a checkpoint and hooks that this transformers version no longer feeds (three positional inputs).

Fixture: q / k / v of two images (1, H, N, D) f32, the out_proj weight and bias, and the two scores.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
import PIL.Image  # noqa: F401  (clip_i.py's ImageType alias reads PIL.Image after a bare `import PIL`)

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.dont_write_bytecode = True

from transformers import BitImageProcessor, CLIPModel, CLIPProcessor, Dinov2Model      # noqa: E402,F401  (resolved before any stub exists)

stubbed = []
for name in ("fire", "megfile", "tqdm", "tqdm.auto", "torchvision", "torchvision.transforms"):       # only where the package is missing
    try:
        __import__(name)
    except ImportError:
        m = types.ModuleType(name)
        m.tqdm = lambda x, *a, **k: x
        m.transforms = None
        sys.modules[name] = m
        stubbed.append(name)
sys.path.insert(0, REF)

from metrics.clip_i import CLIPScore          # noqa: E402
from metrics.dino import Dinov2Score          # noqa: E402

for name in stubbed:                           # (transformers probes optional packages lazily: leave no stub behind)
    del sys.modules[name]


def main():
    H, N, D = 2, 26, 64
    C = H * D
    g = torch.Generator().manual_seed(11)
    q, k, v = ([torch.randn(1, H, N, D, generator=g) * (1.2 if j < 2 else 1.0) for _ in range(2)] for j in range(3))
    out_proj = torch.nn.Linear(C, C)
    with torch.no_grad():
        out_proj.weight.copy_(torch.randn(C, C, generator=g) / C ** 0.5)
        out_proj.bias.copy_(0.1 * torch.randn(C, generator=g))
    clip, dino = object.__new__(CLIPScore), object.__new__(Dinov2Score)

    def mean_cos(ab, ba, aa, bb):
        a_on_b = F.cosine_similarity(ab.reshape(-1).unsqueeze(0), aa.reshape(-1).unsqueeze(0))
        b_on_a = F.cosine_similarity(ba.reshape(-1).unsqueeze(0), bb.reshape(-1).unsqueeze(0))
        return (a_on_b + b_on_a) / 2
    with torch.no_grad():
        cc = lambda x, y: CLIPScore.attention_calc(clip, q[x], k[y], v[y], 0.0, False, D ** -0.5, (1, N, C), out_proj)
        dc = lambda x, y: Dinov2Score.attention_calc(dino, q[x], k[y], v[y], D, torch.nn.Identity())
        s_clip = mean_cos(cc(0, 1), cc(1, 0), cc(0, 0), cc(1, 1))
        s_dino = mean_cos(dc(0, 1), dc(1, 0), dc(0, 0), dc(1, 1))
    np.savez(os.path.join(HERE, "g11_vit_tails.npz"), q=torch.cat(q).numpy(), k=torch.cat(k).numpy(), v=torch.cat(v).numpy(),
             w_out=out_proj.weight.detach().numpy(), bias=out_proj.bias.detach().numpy(), clip_cross=s_clip.numpy(),
             dino_cross=s_dino.numpy())
    print("clip_cross", float(s_clip), "dino_cross", float(s_dino))


if __name__ == "__main__":
    main()
