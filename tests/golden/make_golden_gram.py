#!/usr/bin/env python3
"""Generate g13_gram.npz by running the REFERENCE's own ``gram_matrix`` and ``gram_similarity`` of the gram metric.

Runs only where the reference checkout is (/root/reference); only the data file it writes travels.  metrics/vgg_gram.py imports
torchvision (absent): make_golden.py's name-only stubs are registered for it, plus an empty ``torchvision.models``.  The class is
built without its ``__init__`` (which downloads VGG-19); ``gram_matrix`` (vgg_gram.py:57-69) executes unmodified on seeded features,
and so does ``gram_similarity`` (vgg_gram.py:71-81, line 81 the cosine of ``style_grams[-1]``: the LAST ROW of each Gram matrix) with
``load_image`` and ``get_features`` replaced by the identity, so that its two "paths" are the seeded features themselves.

Fixture: seeded features of two images (1, 32, 5, 7), the reference's two Gram matrices (32, 32) and its score (1,) -- all float64:
the reference's two functions take whatever dtype they are handed, and float64 features make its numbers a yardstick that the
restatement tests/_gram64.py is held to at 1e-10.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden          # noqa: E402  (the stub recipe)


def main():
    make_golden.install_stubs()
    sys.modules["torchvision"].models = sys.modules["torchvision.models"] = types.ModuleType("torchvision.models")
    from metrics.vgg_gram import vgg_gram
    ref = vgg_gram.__new__(vgg_gram)
    ref.device, ref.vgg = "cpu", None
    ref.load_image = lambda path, img_size=512: path
    ref.get_features = lambda image, model, layers=None: image
    g = torch.Generator().manual_seed(13)
    fa = torch.randn(1, 32, 5, 7, generator=g, dtype=torch.float64) * 1.3 + 0.4
    fb = 0.5 * fa + 0.8 * torch.randn(1, 32, 5, 7, generator=g, dtype=torch.float64)
    ga, gb = ref.gram_matrix(fa), ref.gram_matrix(fb)
    score = ref.gram_similarity(fa, fb)
    np.savez(os.path.join(HERE, "g13_gram.npz"), feats_a=fa.numpy(), feats_b=fb.numpy(), gram_a=ga.numpy(), gram_b=gb.numpy(),
             gram=score.numpy())
    full = torch.nn.functional.cosine_similarity(ga.reshape(1, -1), gb.reshape(1, -1))
    print("gram", float(score), tuple(score.shape), "whole matrices", float(full))


if __name__ == "__main__":
    main()
