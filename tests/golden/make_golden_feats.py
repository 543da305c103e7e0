#!/usr/bin/env python3
"""Generate g12_feats.npz by running the REFERENCE's own ``min_max_normalize`` and final cosine of the diffeats metric.

Runs only where the reference checkout is (/root/reference); only the data file it writes travels.  metrics/diffeats.py imports
diffusers, torchvision, seaborn and matplotlib: make_golden.py's name-only stubs are registered for them, plus
``diffusers.models.unets.unet_2d_blocks``, which only diffeats.py names.  ``min_max_normalize`` (diffeats.py:136-140) then executes
unmodified on seeded features, followed by the cosine of diffeats.py:205, restated here line for line because the function around it
needs a pipeline and two U-Net forwards.

Fixture: seeded features of two images (2, 9, 32) f32 (the hook's [B][N][C] output), the reference's normalised tensors, the cosine.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden          # noqa: E402  (the stub recipe)


def main():
    make_golden.install_stubs()

    class _Dummy:
        pass
    sys.modules["diffusers.models.unets"] = types.ModuleType("diffusers.models.unets")
    blocks = types.ModuleType("diffusers.models.unets.unet_2d_blocks")
    blocks.CrossAttnUpBlock2D = blocks.CrossAttnDownBlock2D = blocks.UNetMidBlock2DCrossAttn = _Dummy
    sys.modules["diffusers.models.unets.unet_2d_blocks"] = blocks
    from metrics.diffeats import min_max_normalize
    g = torch.Generator().manual_seed(12)
    fa = torch.randn(2, 9, 32, generator=g) * 1.7 + 0.3
    fb = 0.6 * fa + 0.4 * torch.randn(2, 9, 32, generator=g)
    ga, gb = min_max_normalize(fa), min_max_normalize(fb)
    score = F.cosine_similarity(ga.reshape(-1).unsqueeze(0), gb.reshape(-1).unsqueeze(0))          # diffeats.py:205
    np.savez(os.path.join(HERE, "g12_feats.npz"), feats_a=fa.numpy(), feats_b=fb.numpy(), norm_a=ga.numpy(), norm_b=gb.numpy(),
             diffeats=score.numpy())
    print("diffeats", float(score), tuple(score.shape))


if __name__ == "__main__":
    main()
