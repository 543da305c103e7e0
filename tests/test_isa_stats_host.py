"""tools/isa_stats.py --compare on synthetic assembly: a kernel is compared over its whole body, not up to its first s_endpgm, and
a pure renaming of registers is told apart from a change of the instruction sequence."""
import importlib.util
import os

import pytest

_K = """\t.text
\t.globl\t{name}
{name}:
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_cmp_gt_u32_e32 vcc, 64, v0
\ts_and_saveexec_b64 s[2:3], vcc
\ts_cbranch_execz .LBB0_2
; %bb.1:
\tv_mov_b32_e32 {reg}, 0
\tglobal_store_dword {reg}, {reg}, s[0:1]
\ts_endpgm
.LBB0_2:
\ts_barrier
\tv_mov_b32_e32 v2, {tail}
\tglobal_store_dword v0, v2, s[0:1]
\ts_endpgm
.Lfunc_end0:
\t.size\t{name}, .Lfunc_end0-{name}
"""
_META = """amdhsa.kernels:
  - .agpr_count:     0
    .group_segment_fixed_size: 0
    .name:           {name}
    .private_segment_fixed_size: 0
    .sgpr_count:     12
    .vgpr_count:     3
    .vgpr_spill_count: 0
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
"""


def _asm(reg="v1", tail="1.0", name="_Z4kernPf"):
    return _K.format(name=name, reg=reg, tail=tail) + _META.format(name=name)


@pytest.fixture(scope="module")
def tool():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "isa_stats.py")
    spec = importlib.util.spec_from_file_location("isa_stats", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _compare(tool, tmp_path, capsys, before, after):
    a, b = tmp_path / "before.s", tmp_path / "after.s"
    a.write_text(before)
    b.write_text(after)
    status = tool.compare(str(a), str(b))
    return status, capsys.readouterr().out


def test_compare_reads_past_an_early_endpgm(tool, tmp_path, capsys):
    """two versions that differ only in the block laid out AFTER the first s_endpgm: 'differs', exit status 1"""
    status, out = _compare(tool, tmp_path, capsys, _asm(tail="1.0"), _asm(tail="2.0"))
    assert status == 1
    assert "differs: " in out and "1 differ" in out and "0 identical (" in out, out
    k = tool.kernels(_asm())["_Z4kernPf"][0]
    assert k.count("s_endpgm") == 2 and "s_barrier" in k and not any(ln.startswith(".Lfunc_end") or ln.startswith(".size") for ln in k), k


def test_compare_register_renaming_is_its_own_class(tool, tmp_path, capsys):
    """two versions that differ only in a register name: 'identical up to register names' (still exit status 1); the same text:
    'identical', exit status 0"""
    status, out = _compare(tool, tmp_path, capsys, _asm(reg="v1"), _asm(reg="v2"))
    assert status == 1
    assert "identical up to register names: " in out and "differs: " not in out, out
    assert "1 identical up to register names, 0 differ" in out, out
    status, out = _compare(tool, tmp_path, capsys, _asm(), _asm())
    assert status == 0 and "1 identical (" in out and "0 identical up to register names, 0 differ" in out, out
