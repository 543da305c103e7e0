"""Helpers of the extent tests (tests/test_extent_host.py, tests/test_gpu_extent.py): launches whose operands end just under the
2 GiB that the 32-bit buffer offsets of csrc/gemm.hip and csrc/rowres.hip admit.  Not a conftest: import it like tests/_gemm64.py.

THE METHOD.  A 2 GiB output cannot be held to float64 element by element in seconds, but it can be checked everywhere:
  * the activation (and the residual) is PERIODIC in rows, row r = row r mod P (periodic_rows(): the first P rows are drawn, the
    rest filled with expand + copy_ on the device).  Every output element's K loop is the same whatever its tile or row, so the
    stored output must be periodic BIT FOR BIT: periodic_ok() compares every whole period with period 0 and the ragged last period
    with its prefix, on the device, through integer views and torch.equal;
  * period 0, and required_rows() of the whole range -- the first and last row, the whole last M tile, the rows around the byte
    offsets 2^30 and 2^31 - one tile of rows in the activation and in the output, 64 random rows -- are held to the float64
    reference and bound of tests/_gemm64.py (or to the bit, tests/_rowres64.py's lattice family);
  * sentinels_ok(): the fill value survives in the columns N..ldo, in the gaps between out_split tensors and in the guard rows.
A row read or written at a wrong address anywhere in the 2 GiB breaks the periodicity, a sentinel or the subset bound.  No
tolerance is introduced here."""
import torch

LIMIT = 0x7fffffff           # the launchers refuse a tensor of LIMIT bytes or more
TILE_HEIGHTS = (64, 128, 256, 512)      # every tile height of the GEMM plan table (common.h kSkinnyTiles, gemm.hip gemm_compiled)
PERIOD = 4096                # rows per period of the linears


def bound_rows(row_bytes, fixed_bytes=0, copies=1):
    """(M, M_refused).  M: the largest row count with copies * (M row_bytes + fixed_bytes) <= LIMIT - 1 -- floor((LIMIT - 1) /
    row_bytes) for one tensor -- lowered, if need be, to leave a ragged last tile for every height of TILE_HEIGHTS; M_refused: the
    smallest row count the extent check must refuse (the unadjusted count + 1)."""
    m0 = ((LIMIT - 1) // copies - fixed_bytes) // row_bytes
    m = m0
    while any(m % t == 0 for t in TILE_HEIGHTS):
        m -= 1
    return m, m0 + 1


def bound_images(image_bytes):
    """(B, B_refused) of a conv whose tensor of B images of image_bytes ends at the bound"""
    b = (LIMIT - 1) // image_bytes
    return b, b + 1


def required_rows(M, tile, row_bytes=(), n_random=64, seed=0):
    """The rows of [0, M) that are held to float64 beside period 0: first and last; every row of the last `tile`-row M tile; the
    row that holds byte offset b, and the rows on either side of it, for b = 2^30 and 2^31 - tile rows, per row size of row_bytes
    (the activation's and the output's); n_random seeded random rows.  Sorted unique int64 tensor."""
    sel = [0, M - 1] + list(range((M - 1) // tile * tile, M))
    for rb in row_bytes:
        for b in (1 << 30, (1 << 31) - tile * rb):
            r = b // rb
            sel += [r - 1, r, r + 1]
    g = torch.Generator().manual_seed(seed)
    r = torch.cat([torch.tensor(sel, dtype=torch.int64), torch.randint(0, M, (n_random,), generator=g)])
    return torch.unique(r[(r >= 0) & (r < M)])


def periodic_rows(base, M):
    """[M][...] on base's device with row r = base[r mod P], P = base.shape[0]: expand + copy_, nothing drawn twice"""
    P = base.shape[0]
    out = torch.empty((M,) + tuple(base.shape[1:]), dtype=base.dtype, device=base.device)
    nfull, rem = divmod(M, P)
    if nfull:
        out[:nfull * P].view(nfull, *base.shape).copy_(base.unsqueeze(0).expand(nfull, *base.shape))
    if rem:
        out[nfull * P:].copy_(base[:rem])
    return out


def _words(flat, unit_bytes):
    """a contiguous 1-D tensor as the widest integers that divide unit_bytes (every piece compared is a multiple of it) and its address"""
    for it, w in ((torch.int64, 8), (torch.int32, 4), (torch.int16, 2)):
        if unit_bytes % w == 0 and flat.data_ptr() % w == 0 and flat.element_size() <= w:
            return flat.view(it), w // flat.element_size()
    return flat.view(torch.uint8), 1


def periodic_ok(flat, M, row, P, chunk=64):
    """flat: a contiguous 1-D tensor whose first M * row elements are M rows.  True iff row r equals row r mod P bit for bit for every
    r: whole periods against period 0, `chunk` periods per comparison, and the ragged last period against its prefix."""
    nfull, rem = divmod(M, P)
    if nfull == 0:
        return True
    w, k = _words(flat[:M * row], row * flat.element_size())
    if k == 1 and w.dtype == torch.uint8:
        k, row_w = 1, row * flat.element_size()
    else:
        row_w = row // k
    per = P * row_w
    first = w[:per]
    for i in range(1, nfull, chunk):
        n = min(chunk, nfull - i)
        if not torch.equal(w[i * per:(i + n) * per].view(n, per), first.unsqueeze(0).expand(n, per)):
            return False
    return rem == 0 or torch.equal(w[nfull * per:nfull * per + rem * row_w], w[:rem * row_w])


def periodic_bad_rows(flat, M, row, P, limit=8, chunk_bytes=1 << 26):
    """the first `limit` rows that differ from their image in period 0 (for the failure message): rows r0 .. r1 against rows
    (r0 .. r1) mod P, chunk_bytes of rows per comparison whatever the period"""
    bad = []
    rows = flat[:M * row].view(M, row).view(torch.uint8)
    step = max(1, chunk_bytes // rows.shape[1])
    for r0 in range(P, M, step):
        idx = torch.arange(r0, min(r0 + step, M), device=flat.device)
        ne = (rows[idx] != rows[idx % P]).any(1).nonzero().flatten()
        bad += [r0 + int(v) for v in ne[:limit - len(bad)]]
        if len(bad) >= limit:
            break
    return bad


def out_layout(M, ldo, nout=1, gap=512, guard_rows=4):
    """(elements, per): nout output tensors of M rows of ldo elements, `gap` elements between them when nout > 1 (per: elements from
    one tensor's start to the next's), guard_rows rows of ldo behind the last -- tests/test_gpu_gemm64.py's buffer"""
    per = M * ldo + (gap if nout > 1 else 0)
    return nout * per + guard_rows * ldo, per


def sentinels_ok(out, M, ldo, cols, nout, per, sent):
    """the fill value `sent` (rounded to out's dtype, as torch.full rounded it) still stands in the columns cols..ldo of every
    tensor, between the tensors and behind the last one; compared on out's device.  Returns the name of the first region that was
    written, or None."""
    s = torch.tensor(sent, dtype=out.dtype, device=out.device)
    for j in range(nout):
        blk = out[j * per:j * per + M * ldo].view(M, ldo)
        if cols < ldo and not bool((blk[:, cols:] == s).all()):
            return f"columns {cols}..{ldo} of tensor {j}"
        if not bool((out[j * per + M * ldo:(j + 1) * per] == s).all()):
            return f"the gap behind tensor {j}"
    if not bool((out[nout * per:] == s).all()):
        return "the guard rows past M"
    return None
