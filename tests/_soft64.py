"""A float64 restatement of the soft region score (include/diffsim_amd.h, dsim_pair_score_weights), shared by the soft region tests.
Not a conftest: import it like tests/_region64.py, which it equals exactly where every weight byte is 0 or 255.

Every image i has a byte m_i[t] per token, w = m / 255.  Per pair and direction the rows of non-zero weight are index_select-ed in
ascending token order (a zero-weight row is never touched), the two SDPAs run in float64 with ln w of the key image's rows added to
the logits, their outputs are rounded to the pipeline dtype, and the weighted products and sums are float64: tests/_tail64.py's
products64 on the outputs scaled by sqrt(w) per query row, which puts w on every term of the dot, the two squared norms and the
squared difference; the mse count B H D sum(w) takes sum(w) as (sum of bytes) / 255."""
import torch

from tests._tail64 import SCORE_BUDGET, heads64, products64, sdpa64


@torch.no_grad()
def sdpa64_biased(q, k, v, bias):
    """tests/_tail64.py's sdpa64 with bias (Nk,) float64 added to every query's logits; bias None: sdpa64 itself"""
    if bias is None:
        return sdpa64(q, k, v)
    Bc, H, Nq, D = q.shape
    Nk = k.shape[2]
    rows = max(1, SCORE_BUDGET // (Bc * H * Nk))
    kt = (k.transpose(-1, -2) * (1.0 / D ** 0.5)).contiguous()
    out = torch.empty(Bc, H, Nq, v.shape[3], dtype=torch.float64, device=q.device)
    for r0 in range(0, Nq, rows):
        s = torch.matmul(q[:, :, r0:r0 + rows], kt) + bias
        out[:, :, r0:r0 + rows] = torch.matmul(torch.softmax(s, dim=-1), v)
    return out


class Soft64:
    """The soft tail over the images of q, k, v ([n][B][N][H*D] in the pipeline dtype out_dtype, any device) with the byte weights
    (n, N) uint8.  The SDPA outputs are kept, so that the pairs of one feature set share them."""

    def __init__(self, q, k, v, weights, H, out_dtype):
        self.q, self.k, self.v = q, k, v
        m = torch.as_tensor(weights).detach().cpu()
        assert m.dtype == torch.uint8
        self.rows = [torch.nonzero(r != 0).flatten() for r in m]                               # (ascending)
        self.w = [r[i].double() / 255.0 for r, i in zip(m, self.rows)]                          # the listed rows' weights
        self.wsum = [float(r.long().sum()) / 255.0 for r in m]
        self.H, self.out_dtype = H, out_dtype
        self._o = {}

    def _sel(self, t, i):
        return heads64(t[i], self.H).index_select(2, self.rows[i])

    def attn(self, i, j):
        """sum_u softmax_u(s(t, u) + ln w_j[u]) V_j[u] over the listed rows, rounded to the pipeline dtype, as float64"""
        if (i, j) not in self._o:
            o = sdpa64_biased(self._sel(self.q, i), self._sel(self.k, j), self._sel(self.v, j), torch.log(self.w[j]))
            self._o[(i, j)] = o.to(self.out_dtype).double()
        return self._o[(i, j)]

    def direction(self, x, y, sim):
        """the per-row terms of the direction x -> y, (|rows of x|,) float64: their sum is the direction's value"""
        r = self.w[x].sqrt().view(1, 1, -1, 1)
        con = products64(self.attn(x, y) * r, self.attn(x, x) * r, sim)[1]
        if sim == "mse":                         # products64 divides by B H n D, n the listed rows: the count is B H D sum(w)
            con = con * (len(self.rows[x]) / self.wsum[x])
        return con

    def pair(self, a, b, sim):
        """the soft region score of (a, b): the mean of the two directions (summed as tests/_region64.py sums them); NaN where an
        image has no weight"""
        if len(self.rows[a]) == 0 or len(self.rows[b]) == 0:
            return float("nan")
        return 0.5 * float(torch.cat([self.direction(x, y, sim) for x, y in ((a, b), (b, a))]).sum())


def soft64(q, k, v, weights, idx_a, idx_b, H, sim, out_dtype):
    """[score] for the pairs (idx_a[p], idx_b[p])"""
    t = Soft64(q, k, v, weights, H, out_dtype)
    return [t.pair(a, b, sim) for a, b in zip(torch.as_tensor(idx_a).tolist(), torch.as_tensor(idx_b).tolist())]
