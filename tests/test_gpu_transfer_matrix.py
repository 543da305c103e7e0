"""The transfer matrix on the GPU (csrc/transfer_matrix.hip behind dsim_region_transfer_matrix; engine.region_transfer_matrix): the
attention mass every gallery image sends into every query's weighted tokens.  A cell is dsim_pair_region_transfer's mirror row of its
pair, so it is checked to the bit against engine.pair_region_transfer over the same cells, against the float64 restatement and
per-entry bound of tests/_transfer64.py, and for what the header promises: a cell depends on its two images and the query's weights
alone, non-finite features surface in their row or column alone, refusals enqueue nothing.

n_a = 2 queries and n_b = 3 gallery images (non-square: a transposed cell index shows), tests/test_gpu_region_matrix.py's features,
tests/test_gpu_transfer.py's weight sets (bytes, binary, full, one-hot) on the query images.

Largest err / bound of the first MI355X run (test_cells_stay_within_the_float64_bound; recorded, not used -- the gate is the bound):
see FIRST_RUN below."""
import ctypes
import functools

import pytest
import torch

from tests import _align64 as A
from tests import _transfer64 as T
from tests.test_gpu_region_matrix import _feats
from tests.test_gpu_transfer import SETS, _onehot_token, _weight_sets

pytestmark = pytest.mark.gpu

B = 2
N_A, N_B = 2, 3
SHAPES = [(256, 2, 160), (144, 2, 72), (256, 4, 40), (64, 4, 32)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CASES = [(N, H, D, dt) for N, H, D in SHAPES for dt in DTYPES]
IDS = [f"{N}-{H}-{D}-{str(dt)[6:]}" for N, H, D, dt in CASES]
SENTINEL = -7.0
# first MI355X run, largest err / bound at (144, 2, 72), the random-byte weights, per dtype and logit scale (1 | 14):
FIRST_RUN = {"float32": (0.0068, 0.0060), "bfloat16": (0.0080, 0.0011), "float16": (0.0062, 0.0017)}


@pytest.fixture(scope="module")
def eng():
    from diffsim_amd import engine
    return engine


def _cells():
    """the pair indices of the cells over torch.cat of the sets, row-major"""
    ia = torch.arange(N_A, dtype=torch.int32).repeat_interleave(N_B).cuda()
    ib = (N_A + torch.arange(N_B, dtype=torch.int32)).repeat(N_A).cuda()
    return ia, ib


@functools.lru_cache(maxsize=None)
def _case(N, H, D, dtype, logit_scale=1.0):
    """One case, computed once: the sets' (q, k), the weight sets on all five images ([set][image][N]; only the queries' rows are read
    by the matrix), and per weight set the matrix's masses"""
    from diffsim_amd import engine
    q, k, _v = _feats(N_A + N_B, 300 + N + D, dtype, N, H, D, logit_scale=logit_scale)
    sets = torch.cat([_weight_sets(N, 500 + N), T.random_bytes(len(SETS), N, 7 + N).unsqueeze(1)], dim=1).cuda()      # (4, 5, N)
    fa, fb = (q[:N_A].contiguous(), k[:N_A].contiguous()), (q[N_A:].contiguous(), k[N_A:].contiguous())
    got = []
    for w in sets:
        mass, st = engine.region_transfer_matrix(fa, fb, w[:N_A].contiguous(), H, return_status=True)
        assert mass.shape == (N_A, N_B, N) and not st.any()
        got.append(mass)
    return {"q": q, "k": k, "fa": fa, "fb": fb, "sets": sets, "got": got}


# ---- 1. the pair form over the same cells, to the bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,D,dtype", CASES, ids=IDS)
def test_every_cell_equals_the_pair_form(eng, N, H, D, dtype):
    c = _case(N, H, D, dtype)
    ia, ib = _cells()
    for s, name in enumerate(SETS):
        want, wst = eng.pair_region_transfer(c["q"], c["k"], c["sets"][s].contiguous(), ia, ib, H, directions=2, return_status=True)
        assert not wst.any()
        assert torch.equal(c["got"][s], want[:, 1].view(N_A, N_B, N)), name


# ---- 2. known values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,D,dtype", [(144, 2, 72, torch.float32), (256, 4, 40, torch.bfloat16), (64, 4, 32, torch.float16)], ids=str)
def test_full_weights_give_one_and_one_hot_weights_give_the_attention_column(eng, N, H, D, dtype):
    """tests/test_gpu_transfer.py's rule: |mass - 1| within the float64 bound of the full set; the one-hot mass against that column of
    pair_align's Pm within the sum of the two bounds"""
    c = _case(N, H, D, dtype)
    qc, kc = c["q"].cpu(), c["k"].cpu()
    ia, ib = _cells()
    attn = eng.pair_align(c["q"], c["k"], ia, ib, H, return_attention=True)[3].cpu().double()       # (cells, 2, N, N)
    for i in range(N_A):
        for j in range(N_B):
            _ref, bound = T.direction_mass64(qc[N_A + j], kc[i], c["sets"][2:, i].cpu(), H)          # the full and the one-hot set
            full, one = c["got"][2][i, j].cpu().double(), c["got"][3][i, j].cpu().double()
            assert bool(((full - 1).abs() <= bound[0]).all()), (i, j)
            _pm, ab = A.direction64(qc[N_A + j], kc[i], H)
            t = _onehot_token(i, N)
            err = (one - attn[i * N_B + j, 1, :, t]).abs()
            assert bool((err <= bound[1] + ab[:, t]).all()), (i, j, (err / (bound[1] + ab[:, t])).max().item())


# ---- 3. a cell depends on its two images and the query's weights alone ------------------------------------------------------------------
@pytest.mark.parametrize("N,H,D,dtype", [(256, 2, 160, torch.bfloat16), (144, 2, 72, torch.float16), (64, 4, 32, torch.float32)], ids=str)
def test_other_weights_other_extents_and_a_repeat_change_nothing(eng, N, H, D, dtype):
    c = _case(N, H, D, dtype)
    fa, fb, w = c["fa"], c["fb"], c["sets"][0, :N_A].contiguous()
    base = c["got"][0]
    assert torch.equal(eng.region_transfer_matrix(fa, fb, w, H), base)                               # a repeat
    w2 = w.clone()
    w2[1] = 255 - w2[1]                                                                              # the other query's weights
    moved = eng.region_transfer_matrix(fa, fb, w2, H)
    assert torch.equal(moved[0], base[0]) and not torch.equal(moved[1], base[1])
    fewer = eng.region_transfer_matrix(fa, tuple(t[:2].contiguous() for t in fb), w, H)              # n_b = 2
    assert torch.equal(fewer, base[:, :2])
    alone = eng.region_transfer_matrix(tuple(t[1:].contiguous() for t in fa), tuple(t[2:].contiguous() for t in fb), w[1:].contiguous(), H)
    assert torch.equal(alone[0, 0], base[1, 2])                                                      # the last cell alone
    with_v = eng.region_transfer_matrix((*fa, fa[0]), (*fb, fb[0]), w, H)                            # (q, k, v) tuples: v is not read
    assert torch.equal(with_v, base)


# ---- 4. non-finite features -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,D,dtype", [(256, 2, 160, torch.bfloat16), (144, 2, 72, torch.float32)], ids=str)
def test_a_nan_is_reported_in_its_row_or_column_alone(eng, N, H, D, dtype):
    """Cell (i, j) reads B_j's q and A_i's k (the definition: B_j's queries over A_i's keys).  A NaN in gallery image 1's q raises
    the status of column 1 alone, a NaN in query 0's k that of row 0 alone; the other cells keep their bits.  A gallery image's k is
    not part of any cell: a NaN there raises nothing and changes nothing."""
    c = _case(N, H, D, dtype)
    (qa, ka), (qb, kb), w = c["fa"], c["fb"], c["sets"][0, :N_A].contiguous()
    base = c["got"][0]
    qb2 = qb.clone()
    qb2[1, 1, N // 2, 3] = float("nan")
    mass, st = eng.region_transfer_matrix((qa, ka), (qb2, kb), w, H, return_status=True)
    assert st.tolist() == [[0, 1, 0], [0, 1, 0]]
    assert torch.equal(mass[:, [0, 2]], base[:, [0, 2]]) and bool(torch.isnan(mass[:, 1, N // 2]).all())
    ka2 = ka.clone()
    ka2[0, 1, N // 2, 3] = float("nan")
    mass, st = eng.region_transfer_matrix((qa, ka2), (qb, kb), w, H, return_status=True)
    assert st.tolist() == [[1, 1, 1], [0, 0, 0]]
    assert torch.equal(mass[1], base[1]) and bool(torch.isnan(mass[0]).all())
    kb2 = kb.clone()
    kb2[1, 1, N // 2, 3] = float("nan")
    mass, st = eng.region_transfer_matrix((qa, ka), (qb, kb2), w, H, return_status=True)
    assert not st.any() and torch.equal(mass, base)


# ---- 5. float64 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logit_scale", [1.0, 14.0])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda v: str(v)[6:])
def test_cells_stay_within_the_float64_bound(dtype, logit_scale):
    """The random-byte weights at (144, 2, 72), ordinary logits and logits scaled by 14, entry by entry against tests/_transfer64.py's
    bound: the gate is the bound itself (ratio <= 1), as tests/test_gpu_transfer.py's.  The largest ratio is printed."""
    N, H, D = 144, 2, 72
    c = _case(N, H, D, dtype, logit_scale)
    qc, kc = c["q"].cpu(), c["k"].cpu()
    worst = 0.0
    for i in range(N_A):
        for j in range(N_B):
            ref, bound = T.direction_mass64(qc[N_A + j], kc[i], c["sets"][0, i].cpu(), H)
            got = c["got"][0][i, j].cpu().double()
            assert torch.isfinite(got).all() and got.min() >= 0 and got.max() <= 1 + 1e-6
            worst = max(worst, ((got - ref).abs() / bound).max().item())
    print(f"transfer matrix {N}-{H}-{D} {str(dtype)[6:]} scale {logit_scale:g}: largest err / bound = {worst:.4f}")
    assert worst <= 1.0


# ---- 6. refusals before enqueue ---------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def test_refusals_enqueue_nothing():
    from diffsim_amd import _lib
    L = _lib.lib()
    N, H, D = 64, 4, 32
    c = _case(N, H, D, torch.bfloat16)
    (qa, ka), (qb, kb), w = c["fa"], c["fb"], c["sets"][0, :N_A].contiguous()
    query = L.dsim_region_transfer_matrix_workspace_bytes
    need = int(query(N_A, N_B, B, H, N, D, _lib.DSIM_BF16))
    assert need == N_A * N_B * B * H * N * 4 + 256                 # f32 [cell][B H][N] and the alignment slack: one direction only
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0

    def call(n_a=N_A, D_=D, dtype=_lib.DSIM_BF16, wsb=need, null=()):
        mass = torch.full((N_A, N_B, N), SENTINEL, device="cuda")
        status = torch.full((N_A, N_B), int(SENTINEL), dtype=torch.int32, device="cuda")
        rc = L.dsim_region_transfer_matrix(_p(qa), _p(ka), None if "weights" in null else _p(w), n_a, _p(qb), _p(kb), N_B, B, H, N, D_, dtype,
                                           None if "mass" in null else _p(mass), _p(status), _p(ws), wsb, None)
        torch.cuda.synchronize()
        return rc, mass, status
    for shape in ((0, N_B, B, H, N, D, _lib.DSIM_BF16), (N_A, 0, B, H, N, D, _lib.DSIM_BF16), (N_A, N_B, B, H, N, 24, _lib.DSIM_BF16),
                  (N_A, N_B, B, H, N, D, 9), (40000, 30000, B, H, N, D, _lib.DSIM_BF16), (N_A, N_B, 300, 300, N, D, _lib.DSIM_BF16),
                  (60000, 5000, 1, 1, 64, 16, _lib.DSIM_BF16)):
        assert query(*shape) == 0, shape
    for kw, text in ((dict(n_a=0), b"invalid"), (dict(D_=24), b"invalid"), (dict(dtype=9), b"invalid"), (dict(null=("weights",)), b"invalid"),
                     (dict(null=("mass",)), b"invalid"), (dict(wsb=need - 257), b"workspace")):
        rc, mass, status = call(**kw)
        assert rc != 0 and text in L.dsim_strerror(rc).lower(), (kw, rc)
        assert bool((mass == SENTINEL).all()) and bool((status == int(SENTINEL)).all()), kw
    rc, mass, status = call(wsb=need - 256)                          # the same call with the workspace it needs
    assert rc == 0 and torch.equal(mass, c["got"][0]) and not status.any()
