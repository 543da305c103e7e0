"""A float64 restatement of the region score (include/diffsim_amd.h, dsim_pair_score_regions), shared by the region tests.  Not a
conftest: import it like tests/_tail64.py, whose heads64, sdpa64 and products64 it is built from (they take Nq != Nk).

Every image i has a token region R_i (a mask row).  Per pair and direction the region's rows are index_select-ed in ascending
token order, the two SDPAs run in float64 on the operands as stored, their outputs are rounded to the pipeline dtype, and the
products and sums are float64: cosine over the flattened (B, H, |R_a|, D) tensors, mse divided by B H |R_a| D."""
import torch

from tests._tail64 import heads64, products64, sdpa64


class Region64:
    """The region tail over the images of q, k, v ([n][B][N][H*D] in the pipeline dtype out_dtype, any device) with the regions
    mask (n, N), non-zero = on.  The SDPA outputs are kept, so that the pairs of one feature set share them."""

    def __init__(self, q, k, v, mask, H, out_dtype):
        self.q, self.k, self.v = q, k, v
        self.rows = [torch.nonzero(m.detach().cpu() != 0).flatten() for m in mask]       # (ascending)
        self.H, self.out_dtype = H, out_dtype
        self._o = {}

    def _sel(self, t, i):
        return heads64(t[i], self.H).index_select(2, self.rows[i])

    def attn(self, i, j):
        """SDPA(Q_i[R_i], K_j[R_j], V_j[R_j]) rounded to the pipeline dtype, as float64 (B, H, |R_i|, D)"""
        if (i, j) not in self._o:
            o = sdpa64(self._sel(self.q, i), self._sel(self.k, j), self._sel(self.v, j))
            self._o[(i, j)] = o.to(self.out_dtype).double()
        return self._o[(i, j)]

    def pair(self, a, b, sim):
        """the region score of (a, b): the mean of the two directions"""
        return 0.5 * float(torch.cat([products64(self.attn(x, y), self.attn(x, x), sim)[1] for x, y in ((a, b), (b, a))]).sum())


def regions64(q, k, v, mask, idx_a, idx_b, H, sim, out_dtype):
    """[score] for the pairs (idx_a[p], idx_b[p])"""
    t = Region64(q, k, v, mask, H, out_dtype)
    return [t.pair(a, b, sim) for a, b in zip(torch.as_tensor(idx_a).tolist(), torch.as_tensor(idx_b).tolist())]
