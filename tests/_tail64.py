"""A float64 restatement of the score tail (the reference's diffsim.py:177-197), shared by the tail tests.  Not a conftest: import it
like tests/_fakes.py.

The semantics are those of the pipeline: the two SDPAs of a direction run in float64 on the operands as the kernels see them (already
rounded to the pipeline dtype), their outputs are rounded to the pipeline dtype, and the products and sums are float64.  Per pair and
direction it keeps the per-token terms of engine.pair_score_maps: local (the token's own cosine, or its mean squared difference) and
contrib (its share of the score), so that score = 0.5 * contrib.sum().

The SDPA runs in query chunks sized to hold about 32 MB of float64 scores, under torch.no_grad(): at 4096 tokens a call needs tens of
MB where one unchunked float64 SDPA would materialise gigabytes."""
import torch

SCORE_BUDGET = 1 << 22          # float64 score elements per query chunk (32 MB)


def heads64(t, H):
    """[B][N][H*D] (any dtype, any device) -> (B, H, N, D) float64 on the CPU"""
    Bc, N, HD = t.shape
    return t.detach().cpu().double().view(Bc, N, H, HD // H).transpose(1, 2).contiguous()


@torch.no_grad()
def sdpa64(q, k, v, chunk=None):
    """softmax(q k^T / sqrt(D)) v in float64 for (B, H, Nq, D) / (B, H, Nk, D) float64 tensors, chunk query rows at a time (default:
    as many as keep a chunk's scores within SCORE_BUDGET elements)"""
    Bc, H, Nq, D = q.shape
    Nk = k.shape[2]
    rows = chunk or max(1, SCORE_BUDGET // (Bc * H * Nk))
    kt = (k.transpose(-1, -2) * (1.0 / D ** 0.5)).contiguous()
    out = torch.empty(Bc, H, Nq, v.shape[3], dtype=torch.float64, device=q.device)
    for r0 in range(0, Nq, rows):
        s = torch.matmul(q[:, :, r0:r0 + rows], kt)
        out[:, :, r0:r0 + rows] = torch.matmul(torch.softmax(s, dim=-1), v)
    return out


def products64(x, o, sim):
    """One direction's per-token terms: x the cross output, o the self output, (B, H, N, D) float64.  Returns (local (N,),
    contrib (N,)); the direction's score is contrib.sum()."""
    Bc, H, N, D = x.shape
    if sim == "cosine":
        dot = (x * o).sum((0, 1, 3))
        x2, y2 = (x * x).sum((0, 1, 3)), (o * o).sum((0, 1, 3))
        local = dot / (x2.sqrt().clamp_min(1e-8) * y2.sqrt().clamp_min(1e-8))     # (F.cosine_similarity's eps)
        contrib = dot / (x2.sum().sqrt().clamp_min(1e-8) * y2.sum().sqrt().clamp_min(1e-8))
    elif sim == "mse":
        sqd = ((x - o) ** 2).sum((0, 1, 3))
        local = sqd / (Bc * H * D)
        contrib = sqd / (Bc * H * N * D)
    else:
        raise ValueError(sim)
    return local, contrib


class Tail64:
    """The tail over the images of q, k, v ([n][B][N][H*D] in the pipeline dtype out_dtype, any device).  SDPA outputs are computed
    once and kept, so that the pairs and the matrix cells of one feature set share them."""

    def __init__(self, q, k, v, H, out_dtype, chunk=None):
        self.q, self.k, self.v = q, k, v
        self.H, self.out_dtype, self.chunk = H, out_dtype, chunk
        self._o = {}

    def attn(self, i, j):
        """SDPA(Q_i, K_j, V_j) rounded to the pipeline dtype, as float64 (B, H, N, D)"""
        if (i, j) not in self._o:
            o = sdpa64(heads64(self.q[i], self.H), heads64(self.k[j], self.H), heads64(self.v[j], self.H), self.chunk)
            self._o[(i, j)] = o.to(self.out_dtype).double()
        return self._o[(i, j)]

    def pair(self, a, b, sim):
        """(score, local (2, N), contrib (2, N)): direction 0 on image a's tokens (O_ab against O_aa), direction 1 on b's"""
        loc, con = zip(*(products64(self.attn(x, y), self.attn(x, x), sim) for x, y in ((a, b), (b, a))))
        con = torch.stack(con)
        return 0.5 * float(con.sum()), torch.stack(loc), con


def pairs64(q, k, v, idx_a, idx_b, H, sim, out_dtype, chunk=None):
    """[(score, local (2, N), contrib (2, N))] for the pairs (idx_a[p], idx_b[p])"""
    t = Tail64(q, k, v, H, out_dtype, chunk)
    return [t.pair(a, b, sim) for a, b in zip(torch.as_tensor(idx_a).tolist(), torch.as_tensor(idx_b).tolist())]


def matrix64(fa, fb, H, sim, out_dtype, chunk=None):
    """(n_a, n_b) float64 scores of every image of set A (q, k, v) against every image of set B"""
    na, nb = fa[0].shape[0], fb[0].shape[0]
    t = Tail64(*(torch.cat([a.cpu(), b.cpu()]) for a, b in zip(fa, fb)), H, out_dtype, chunk)
    return torch.tensor([[t.pair(i, na + j, sim)[0] for j in range(nb)] for i in range(na)], dtype=torch.float64)
