"""The gram metric's arithmetic restated in torch ops, independent of the engine: the conv stack of torchvision's vgg19().features up
to the last conv of a plan (no ReLU behind it), the Gram matrix over the spatial axis, the cosine of the last row (the reference's
``style_grams[-1]``) or of the whole matrices.  float64 is the yardstick; the same functions run in bfloat16 / float16 give the error
torch's own 16-bit arithmetic makes, which the 16-bit gates are stated in (tests/_walk64.py's rule).

State dicts are under torchvision's keys ``features.N.{weight,bias}``; a plan is conv output channels and "P" for a pool."""
import math

import torch
import torch.nn.functional as F

SMALL_PLAN = (64, 64, "P", 128, 128, "P", 256)
VGG19_PLAN = (64, 64, "P", 128, 128, "P", 256, 256, 256, 256, "P", 512, 512, 512, 512, "P", 512)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def conv_indices(plan):
    """torchvision's module index of every conv of the plan: a conv and its ReLU take two slots, a pool one"""
    out, i = [], 0
    for e in plan:
        if e == "P":
            i += 1
        else:
            out.append(i)
            i += 2
    return out


def he_state_dict(plan, seed=0, in_channels=3):
    """He-initialised f32 weights and small biases under torchvision's keys"""
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, in_channels
    for idx, cout in zip(conv_indices(plan), [e for e in plan if e != "P"]):
        sd[f"features.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        sd[f"features.{idx}.bias"] = torch.randn(cout, generator=g) * 0.1
        cin = cout
    return sd


def features(pixels, sd, plan, dtype=torch.float64):
    """(n, C, H', W') in `dtype`: conv3x3 + bias, ReLU behind every conv but the last, MaxPool2d(2, 2) in floor mode"""
    x = pixels.to(dtype)
    idx = conv_indices(plan)
    convs = [e for e in plan if e != "P"]
    j = 0
    for e in plan:
        if e == "P":
            x = F.max_pool2d(x, 2, 2)
            continue
        x = F.conv2d(x, sd[f"features.{idx[j]}.weight"].to(dtype), sd[f"features.{idx[j]}.bias"].to(dtype), padding=1)
        j += 1
        if j < len(convs):
            x = F.relu(x)
    return x


def gram_matrix(feat):
    """vgg_gram.py:57-69 for one image (1, C, H, W): X X^T with X = feat.view(C, H W), not normalised"""
    b, d, h, w = feat.shape
    x = feat.reshape(b * d, h * w)
    return x @ x.t()


def cosine(a, b, eps=1e-8):
    """F.cosine_similarity of two flat vectors as torch computes it: x . y / (max(|x|, eps) max(|y|, eps))"""
    a, b = a.reshape(-1), b.reshape(-1)
    return (a @ b) / (a.norm().clamp_min(eps) * b.norm().clamp_min(eps))


def score(gram_a, gram_b, full=False):
    """vgg_gram.py:81: the cosine of the LAST ROWS of the two Gram matrices; full: of the whole matrices"""
    return cosine(gram_a, gram_b) if full else cosine(gram_a[-1], gram_b[-1])


def similarity_of_features(feat_a, feat_b, full=False):
    """steps 3-4 on given features (1, C, H, W)"""
    return score(gram_matrix(feat_a), gram_matrix(feat_b), full)


def normalise(rgb_u8):
    """ToTensor + Normalize of a uint8 (H, W, 3) array -> (1, 3, H, W) float64"""
    x = torch.from_numpy(rgb_u8.copy()).to(torch.float64) / 255.0
    x = (x - torch.tensor(MEAN, dtype=torch.float64)) / torch.tensor(STD, dtype=torch.float64)
    return x.permute(2, 0, 1)[None]


def similarity(pix_a, pix_b, sd, plan, full=False, dtype=torch.float64):
    """steps 2-4 for two normalised images; the Gram product and the cosine run in float64 on the `dtype` features"""
    ga = gram_matrix(features(pix_a, sd, plan, dtype).to(torch.float64))
    gb = gram_matrix(features(pix_b, sd, plan, dtype).to(torch.float64))
    return score(ga, gb, full)
