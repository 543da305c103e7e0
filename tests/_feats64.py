"""A float64 restatement of the two feature-cosine metrics from q, k, v, shared by the feature tests.  Not a conftest: import it like
tests/_tail64.py.

  diffeats  (reference metrics/diffeats.py:136-205, hook metrics/hooks.py:37-38): F = to_out.0(merge_heads(SDPA(q, k, v))) + bias over
            both CFG halves, G = (F - min F) / (max F - min F) over all B N C values (diffeats.py:136-140), score =
            cosine_similarity(flat G_a, flat G_b), eps 1e-8 (:205).
  dinofeats (reference metrics/dino.py:163-183, hook metrics/hooks.py:34-35): F = merge_heads(SDPA(q, k, v)), the context layer, class
            token included; no projection, no normalisation; the same cosine.

The rounding points are the pipeline's: the attention outputs, the projection and the normalised values are each rounded to the
pipeline dtype (the normalisation through float32, as the kernel divides in f32); everything between them is float64.  restate() is
the same arithmetic as plain torch ops IN the pipeline dtype, the yardstick the tests size their bounds with."""
import torch
import torch.nn.functional as F

from tests._tail64 import heads64, sdpa64


def min_max_normalize64(x, out_dtype):
    """diffeats.py:136-140 on a float64 tensor; the quotient rounded to float32, then to the pipeline dtype"""
    mn, mx = x.min(), x.max()
    return ((x - mn) / (mx - mn)).float().to(out_dtype).double(), float(mn), float(mx)


def features64(q, k, v, H, out_dtype, w_out=None, bias=None, minmax=False):
    """q, k, v [n][B][N][H*D] in the pipeline dtype -> (G float64 [n][B][N][C], stats float64 [n][3] = sum of G^2, min F, max F)"""
    out, stats = [], []
    for i in range(q.shape[0]):
        o = sdpa64(heads64(q[i], H), heads64(k[i], H), heads64(v[i], H)).to(out_dtype).double()          # (B, H, N, D)
        f = o.transpose(1, 2).reshape(o.shape[0], o.shape[2], -1)                                         # merge_heads
        if w_out is not None:
            f = (f @ w_out.detach().cpu().double().T + bias.detach().cpu().double()).to(out_dtype).double()
        mn, mx = float(f.min()), float(f.max())
        if minmax:
            f, mn, mx = min_max_normalize64(f, out_dtype)
        out.append(f)
        stats.append([float((f * f).sum()), mn, mx])
    return torch.stack(out), torch.tensor(stats, dtype=torch.float64)


def cosine64(a, b):
    """F.cosine_similarity(flat a, flat b), eps 1e-8, in float64"""
    a, b = a.reshape(-1).double(), b.reshape(-1).double()
    return float((a * b).sum() / (a.norm().clamp_min(1e-8) * b.norm().clamp_min(1e-8)))


def matrix64(ga, gb):
    """(n_a, n_b) float64 cosines of every image of ga against every image of gb ([n][...] features)"""
    a, b = ga.reshape(ga.shape[0], -1).double().cpu(), gb.reshape(gb.shape[0], -1).double().cpu()
    return (a @ b.T) / (a.norm(dim=1).clamp_min(1e-8)[:, None] * b.norm(dim=1).clamp_min(1e-8)[None, :])


def restate(q, k, v, H, w_out=None, bias=None, minmax=False):
    """The same features as plain torch ops in the tensors' own dtype on the CPU (SDPA, linear, min-max normalise, as the
    reference's modules run them): [n][B][N][C] in that dtype"""
    n, B, N, HD = q.shape
    hd = lambda t: t.detach().cpu().view(n * B, N, H, HD // H).transpose(1, 2)
    f = F.scaled_dot_product_attention(hd(q), hd(k), hd(v)).transpose(1, 2).reshape(n, B, N, HD)
    if w_out is not None:
        f = F.linear(f, w_out.detach().cpu(), bias.detach().cpu().to(f.dtype))
    if minmax:
        f = torch.stack([(x - x.min()) / (x.max() - x.min()) for x in f])
    return f
