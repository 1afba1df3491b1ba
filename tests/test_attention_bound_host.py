"""CPU: the element-wise bound of the attention edge tests (tests/attention_cases.py) is validated from the reference alone, for
both activation types, so that the tolerance of tests/test_gpu_attention_edges.py is never fitted to the kernel:
  - a float64 model of the kernel's two roundings stays inside half the bound everywhere;
  - four mutants of the reference (what a subtly wrong kernel computes) each leave the bound in at least one element of every case
    that exercises the feature they break -- a case in which a mutant stayed inside would be blind to that bug."""
import pytest
import torch

from tests import attention_cases as AC

ADTS = [torch.float16, torch.bfloat16]
_cache = {}


def _data(case, adt):
    key = (case.name, adt)
    if key not in _cache:
        q, k, v, bias = AC.make_inputs(case, adt)
        ref, bound = AC.reference(q, k, v, bias, case.heads, adt)
        _cache[key] = (q, k, v, bias, ref, bound)
    return _cache[key]


def test_case_table_covers_the_edges():
    """The table itself: every head dim below a class top with >= 2 heads, the three stride patterns, the query and key edges, both
    query-tile forms at Nq = 130, and the product's mask shapes."""
    cs = AC.CASES
    assert {8, 16, 24, 40, 56, 72, 88} <= {c.dh for c in cs if c.heads >= 2}
    assert any(c.Nq == 130 and c.Nk == 77 for c in cs)
    assert {"plain", "qkv", "ctx"} == {c.layout for c in cs}
    assert all((c.ldq, c.ldk, c.ldv) == (3 * c.heads * c.dh,) * 3 and c.Nq == c.Nk for c in cs if c.layout == "qkv")
    assert all(c.ldq == c.heads * c.dh and c.ldk == c.ldv == 2 * c.heads * c.dh + 8 for c in cs if c.layout == "ctx")
    assert {1, 63, 64, 65, 127, 128, 129, 130} <= {c.Nq for c in cs}
    assert {1, 8, 50, 63, 64, 65, 128, 129, 200} <= {c.Nk for c in cs}
    assert any(c.Nq == 130 and c.B * c.heads >= 129 and c.qt == 2 for c in cs) and any(c.Nq == 130 and c.qt == 1 for c in cs)
    assert any(c.inp == "peaked" for c in cs) and any(c.inp == "ends" for c in cs) and any(c.Nk >= 512 for c in cs)
    assert any(c.Nk == 200 and c.mask == (8, 198) for c in cs) and any(c.Nk == 130 and c.mask == (1, 127) for c in cs)
    assert any(c.mask == (0, 63) and c.Nk > 64 for c in cs)
    for c in cs:
        if c.mask is not None:
            b = AC.make_bias(c)
            assert (b[:, -1] == 0).all() and set(b.unique().tolist()) == {-10000.0, 0.0}
            assert (b[:, 0] == 0).all() or c.mask[0] == 0
        if c.Nk >= 512:
            assert (AC.make_inputs(c, torch.float16)[2][:, -1] == 4).all()


@pytest.mark.parametrize("adt", ADTS, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", AC.CASES, ids=[c.name for c in AC.CASES])
def test_emulated_kernel_stays_inside_half_the_bound(case, adt):
    q, k, v, bias, ref, bound = _data(case, adt)
    emu = AC.emulate(q, k, v, bias, case.heads, adt)
    ratio = ((emu - ref).abs() / bound).max().item()
    print(f"{case.name} {adt}: emulated err / (3u + sub) = {ratio:.3f}")
    assert torch.isfinite(emu).all() and ratio <= 0.5, ratio


@pytest.mark.parametrize("adt", ADTS, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", AC.CASES, ids=[c.name for c in AC.CASES])
def test_every_applicable_mutant_leaves_the_bound(case, adt):
    q, k, v, bias, ref, bound = _data(case, adt)
    applied = []
    for name, fn in AC.MUTANTS.items():
        mut = fn(case, q, k, v, bias)
        if mut is None:
            continue
        ratio = ((mut - ref).abs() / bound).max().item()
        print(f"{case.name} {adt}: mutant {name} err / (3u + sub) = {ratio:.2f}")
        applied.append(name)
        assert ratio > 1.0, (name, ratio)
    assert applied or case.Nk < 2


def test_each_mutant_is_applied_somewhere():
    for name, fn in AC.MUTANTS.items():
        hits = [c.name for c in AC.CASES if fn(c, *AC.make_inputs(c, torch.float16)) is not None]
        assert hits, name
    q, k, v, bias = AC.make_inputs(AC.BY_NAME["dh8"], torch.float16)
    assert AC.mutant_ignore_one_bias(AC.BY_NAME["dh8"], q, k, v, bias) is None
    assert AC.mutant_key_row_off_by_one(AC.BY_NAME["dh8"], q, k, v, bias) is None
    assert AC.mutant_next_head_channels(AC.BY_NAME["nq1"], *AC.make_inputs(AC.BY_NAME["nq1"], torch.float16)) is None
