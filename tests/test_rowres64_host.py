"""CPU checks of tests/_rowres64.py, what tests/test_gpu_rowres64.py holds the row-resident kernels (csrc/rowres.hip) to: the lattice
family meets its own conditions for every small (M, seed) the GPU test uses, and a CPU replay of the kernels' rounding points
reproduces its expected output bit for bit; the same replay on ordinary data lies inside the float64 bound; every listed mutation of
the replay -- what a bug in the weight stream, the ring, the tile loop or the epilogue would compute -- changes the lattice output
and is rejected by the float64 bound (bf16 exceptions by name); the bound passes the rounded reference and fails a two-ulp move; and
the product library holds exactly the ff_fused_kernel / rowlin_kernel instantiations the GPU test runs."""
import pytest
import torch

from tests import _gemm64 as G
from tests import _norm64 as N
from tests import _rowres64 as R
from tests import test_gpu_rowres64 as T

DT = T.DT
EPS = 1e-5
_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def _lat(M, dt):
    return _once(("lat", M, dt), lambda: R.lattice(M, DT[dt], M, "cpu"))


# ---- the family ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("M", sorted(set(T.FF_SMALL_M + (T.LIN_M,))))
def test_lattice_conditions_and_replay_to_the_bit(M, dt):
    """lattice() asserts its conditions itself (check_conditions); here also: the rowres LayerNorm emulation returns n = beta +
    sigma gamma bit for bit, and the replays of both chains return the expected outputs bit for bit"""
    dtype = DT[dt]
    t = _lat(M, dt)
    c = t["cond"]
    R.check_conditions(c)
    assert c["gmin"] >= 11.0 and c["s2"] * 2.0 ** 7 <= 2.0 ** 23 and c["absmax"] < 4096, c
    n = N.emulate_layernorm(t["x"], t["gamma"], t["beta"], EPS, dtype, dict(form="rowres"))
    assert torch.equal(R.bits(n), R.bits(t["n"]))
    assert torch.equal(t["n"].double(), t["beta"].double() + t["sigma"] * t["gamma"].double())
    assert t["n"].double().abs().min() >= 0.5
    R.assert_bits(R.replay_ff(t["x"], *R.ff_args(t), EPS, dtype), t["ff"], "replay_ff")
    for ln in (True, False):
        out, _ = R.replay_rowlin(t["x"], t["gamma"] if ln else None, t["beta"], t["wl"], EPS, dtype)
        R.assert_bits(out, t["lin_ln"] if ln else t["lin"], f"replay_rowlin ln={ln}")
    if M > 32:
        assert t["ff"].float().unique().numel() > 1000              # not a handful of values that a wrong sum could hit by chance


def test_lattice_is_a_function_of_its_arguments():
    a, b, c = R.lattice(33, torch.float16, 7), R.lattice(33, torch.float16, 7), R.lattice(33, torch.float16, 8)
    assert all(torch.equal(a[k], b[k]) for k in ("x", "w1", "w2", "wl", "ff", "lin_ln", "lin"))
    assert not torch.equal(a["x"], c["x"]) and not torch.equal(a["w1"], c["w1"])
    x = a["x"].double()
    assert torch.equal(x.sum(1), 320 * x.mean(1)) and set(x.mean(1).tolist()) <= {0.0, 4.0, -4.0}
    assert set((x - x.mean(1, keepdim=True)).abs().unique().tolist()) <= {0.5, 1.0, 2.0}


def test_gelu_fast_is_the_identity_from_8_on():
    """the f32 facts the family's g >= 8 rests on: t <= -39, 1 + exp2(t) == 1"""
    g = torch.arange(16, 80, dtype=torch.float32) / 2
    u = torch.clamp(g * g, max=64.0)
    t = g * (u * (u * 1.01426306e-3 - 0.106775724) - 2.30112134)
    assert t.max() <= -39.0 and torch.equal(1.0 + torch.exp2(t), torch.ones_like(t))
    assert torch.equal(G.gelu_fast64(g.double()).float(), g)


def test_condition_checks_reject_what_they_name():
    good = dict(_lat(33, "f16")["cond"])
    for k, v in (("gmin", 7.5), ("prod_exact", False), ("s2", 2.0 ** 16 + 1), ("absmax", 70000.0), ("cover", (True, False, True))):
        with pytest.raises(AssertionError):
            R.check_conditions(dict(good, **{k: v}))
    w = R.lattice_weights(3)
    w1 = w["w1"].clone()
    w1[R.HID + 32 * 5:R.HID + 32 * 6, 16 * 3:16 * 4] = 0              # one k-step of one g chunk multiplied by nothing
    assert R.weight_coverage(w1, w["w2"]) == (True, False, True)
    w2 = w["w2"].clone()
    w2[64:96, 32 * 9 + 4] = 0
    assert R.weight_coverage(w["w1"], w2) == (True, True, False)


# ---- ordinary data: the replay inside the bound; mutations outside ------------------------------------------------------------------
M_RND = 161
ROWS = torch.cat([torch.arange(0, 24), torch.arange(128, M_RND)])          # both tiles; the Jacobian term costs 0.26 GFLOP a row


def _rnd(dt):
    return _once(("rnd", dt), lambda: R.random_inputs(M_RND, DT[dt], 5))


def _ff_bound(dt):
    t = _rnd(dt)
    return _once(("ffb", dt), lambda: R.ff_ref_and_bound(t["x"], *R.ff_args(t), EPS, DT[dt], rows=ROWS))


@pytest.mark.parametrize("dt", list(DT))
def test_replay_within_bound_on_ordinary_data(dt):
    dtype = DT[dt]
    t = _rnd(dt)
    ref, bound = _ff_bound(dt)
    assert N.check(R.replay_ff(t["x"], *R.ff_args(t), EPS, dtype)[ROWS], ref, bound, f"replay_ff {dt}") <= 1.0
    for Nn in (64, 960):
        out, n = R.replay_rowlin(t["x"], t["gamma"], t["beta"], t["wl"][:Nn], EPS, dtype)
        assert G.Gemm64(n, t["wl"][:Nn], dtype).check(out, f"replay_rowlin {dt} N={Nn}") <= 1.0


def _rows_hit(a, b):
    return int((R.bits(a) != R.bits(b)).any(1).sum())


BF16_BOUND_CANNOT_REJECT = ()          # mutations the bf16 float64 bound lets through: the lattice test is what rejects those


@pytest.mark.parametrize("mut", R.MUTATIONS_FF)
def test_ff_mutations_change_the_lattice_and_leave_the_bound(mut):
    M = T.FF_SMALL_M[-1]
    for dt, dtype in DT.items():
        t = _lat(M, dt)
        hit = _rows_hit(R.replay_ff(t["x"], *R.ff_args(t), EPS, dtype, mut), t["ff"])
        assert hit == (M - R.TILE if mut == "tile1_from_tile0_rows" else M), (mut, dt, hit)
    passes = {}
    for dt, dtype in DT.items():
        t = _rnd(dt)
        ref, bound = _ff_bound(dt)
        passes[dt] = N.excess(R.replay_ff(t["x"], *R.ff_args(t), EPS, dtype, mut)[ROWS], ref, bound) <= 1.0
    assert not passes["f16"], mut
    assert passes["bf16"] == (mut in BF16_BOUND_CANNOT_REJECT), mut


@pytest.mark.parametrize("ln", [True, False])
@pytest.mark.parametrize("mut", R.MUTATIONS_LIN)
def test_rowlin_mutations_change_the_lattice_and_leave_the_bound(mut, ln):
    for dt, dtype in DT.items():
        t = _lat(T.LIN_M, dt)
        out, _ = R.replay_rowlin(t["x"], t["gamma"] if ln else None, t["beta"], t["wl"], EPS, dtype, mut)
        assert _rows_hit(out, t["lin_ln"] if ln else t["lin"]) == T.LIN_M, (mut, dt)
        r = _rnd(dt)
        bad, n = R.replay_rowlin(r["x"], r["gamma"] if ln else None, r["beta"], r["wl"], EPS, dtype, mut)
        with pytest.raises(AssertionError):
            G.Gemm64(n, r["wl"], dtype).check(bad, mut)


@pytest.mark.parametrize("dt", list(DT))
def test_rounded_reference_passes_and_two_ulps_fail(dt):
    """rowlin's bound is the plain GEMM epilogue's: two ulps on its largest element fail.  The chain's bound has an absolute part --
    LAM times the independent roundings of the LayerNorm output and of hid, carried to the output -- that on randn rows (largest
    output about 7) is itself two ulps of the largest element.  The ulp grows with the element and that part does not: with one
    residual outlier in a row (x = 48 in one channel, as an activation outlier is), two ulps on the largest element fail."""
    dtype = DT[dt]
    t = _rnd(dt)
    n = N.emulate_layernorm(t["x"], t["gamma"], t["beta"], EPS, dtype, dict(form="rowres"))
    g = G.Gemm64(n, t["wl"], dtype)
    got = g.ref.to(dtype)
    assert g.check(got, "rowlin") <= 1.0
    r, c = divmod(int(g.ref.abs().argmax()), g.ref.shape[1])
    bad = got.double().clone()
    bad[r, c] += 2 * float(R.ulp(bad[r, c], dtype))
    with pytest.raises(AssertionError):
        g.check(bad.to(dtype), "rowlin")

    x = t["x"][:32].clone()
    x[5, 77] = 48.0
    ref, bound = R.ff_ref_and_bound(x, *R.ff_args(t), EPS, dtype)
    got = ref.to(dtype)
    assert N.check(got, ref, bound, "ff") <= 1.0
    assert N.check(R.replay_ff(x, *R.ff_args(t), EPS, dtype), ref, bound, "ff replay") <= 1.0
    r, c = divmod(int(ref.abs().argmax()), ref.shape[1])
    assert (r, c) == (5, 77)
    bad = got.double().clone()
    bad[r, c] += 2 * float(R.ulp(bad[r, c], dtype))
    assert N.excess(bad.to(dtype), ref, bound) > 1.0


def test_compiled_instantiations_are_the_pair_the_gpu_test_runs():
    """The product library holds ff_fused_kernel<0> and rowlin_kernel<0> once per 16-bit namespace (dsim::bf16, dsim::f16: the
    kernels live in each compilation's anonymous namespace, so the two copies share a name; the launchers that own them do not) and
    no other instantiation: a new one cannot go untested.  Read from the library's kernel-handle symbols."""
    import re
    import shutil
    import subprocess
    from diffsim_amd import build
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    syms = subprocess.run(["nm", build.build()], capture_output=True, text=True, check=True).stdout
    for kern, launcher in (("ff_fused_kernel", "launch_ff_fused"), ("rowlin_kernel", "launch_rowlin")):
        inst = re.findall(rf"^\S+ [dD] _ZN4dsim12_GLOBAL__N_1\d+{kern}ILi(\d+)EEE", syms, re.M)
        assert inst == ["0", "0"], (kern, inst)
        for ns in ("4bf16", "3f16"):
            assert re.search(rf" T _ZN4dsim{ns}\d+{launcher}E", syms), (ns, launcher)
