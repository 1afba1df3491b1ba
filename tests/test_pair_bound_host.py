"""CPU: the two-stage float64 model, the bound and the case table of tests/pair_cases.py are validated from the reference alone, for both
activation types, so that the tolerance of tests/test_gpu_pair_elementwise.py is never fitted to the kernel:
  - the two-stage model equals torch's own float64 conv1d -> leaky_relu -> conv1d + reconstructed residual (forward),
    conv_transpose1d . mask -> conv_transpose1d . mask + residual + previous (backward) and the single-stage builders to 1e-11 relative;
  - an fp32 emulation of the kernel's arithmetic (bias-first accumulators at C < 128 without a mask, the bias in the tail at C = 128, two
    accumulation orders, the intermediate rounded once to 16 bits) stays inside the bound and, beyond the one unavoidable output rounding,
    uses at most half of what the bound leaves (the margin rule of tests/test_gemm_bound_host.py); the sharp reference -- stage b on the
    emulated tape -- holds it with the plain single-launch bound;
  - every mutant of the model leaves the bound in every case that exercises it, and applies somewhere;
  - the ambiguous-sign set of a bits-only tape is at most 1 % of the intermediate, from the reference alone;
  - sharp_fraction is reported per case."""
import pytest
import torch

from tests import gemm_cases as G
from tests import pair_cases as P

ADTS = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
NAMES = [c.name for c in P.CASES]

BUILDERS = {
    "forward": lambda: P.forward_case("b-fwd", 2, 61, 16, 5, 3, tape="both"),
    "forward-executor": lambda: P.forward_case("b-fwd-ex", 2, 61, 16, 5, 3, executor=True),
    "forward-accum-sep-r": lambda: P.forward_case("b-fwd-acc", 2, 61, 16, 5, 3, accum=True, sep_r=True, ldw_pad=8),
    "backward": lambda: P.backward_case("b-bwd", 2, 61, 16, 5, 3),
    "backward-maskbits": lambda: P.backward_case("b-bwd-maskbits", 2, 61, 16, 5, 3, maskbits=True),
    "single": lambda: P.single_case("b-single", 2, 61, 16, 5, 3, G.EPI_BIAS),
    "single-resid-lrelu2": lambda: P.single_case("b-single2", 2, 61, 16, 5, 3, G.EPI_BIAS | G.EPI_RESID | G.EPI_LRELU2),
}


@pytest.mark.parametrize("which", list(BUILDERS))
def test_two_stage_model_is_the_torch_operation(which):
    problems, bufs, tref = BUILDERS[which]()
    outs, _ = P.expected_pair(problems, bufs, None)
    want = tref(bufs)
    assert want
    for name, w in want.items():
        val, _, cnt = outs[name]
        assert (cnt == 1).all(), name
        err = (val.view(w.shape) - w).abs().max().item()
        print(f"{which}: {name} max |model - torch float64| = {err:.2e}")
        assert err < 1e-11 * max(1.0, w.abs().max().item())


def test_slab_arithmetic_of_the_dead_rows():
    """the skip spans of the issue on four slabs: which slabs go, never all"""
    for k, dil, BMo in ((7, 3, 250), (7, 3, 238)):
        T = 3 * BMo + 5
        want = {"slab1": (1, 2), "slab0": (0, 1), "slab2-and-last": (2, 4), "inside-slab0": (0, 0), "whole-clip": (0, 0)}
        for sp, (fn, n) in P.SKIP_SPANS.items():
            assert P.skip_slabs(fn(BMo, T), T, BMo) == want[sp] and want[sp][1] - want[sp][0] == n, sp
    assert [P.fwd_bmo(k) for k, _ in P.GRID] == [254, 250, 246] and [P.bwd_bmo(k, d) for k, d in P.GRID] == [254, 238, 206]


def test_case_table():
    cs = P.CASES
    fwd = [c for c in cs if c.family == "fwd"]
    assert {(c.feat["C"], c.feat["k"], c.feat["dil"]) for c in fwd} == {(C, k, d) for C in P.WIDTHS for k, d in P.GRID}
    for c in fwd:
        p = c.data(torch.float16)[0][0]
        assert p.b.Wq == 2 * P.slab_rows(p.a, p.b) + 3 and p.b.M == 2 * p.b.Wq and p.b.R == p.a.A
    assert {c.feat["variant"] for c in cs if c.family == "fwd-variant"} == {"tape-bits", "tape-both", "executor", "sep-r", "accum", "ldw", "ldb2"}
    assert {c.feat["T"] for c in cs if c.family == "fwd-edge" and c.feat["C"] == 64} == {1, 5, 249, 250, 251}
    assert {(c.feat["C"], c.feat["T"]) for c in cs if c.family == "fwd-edge" and c.feat["C"] != 64} == {(32, 254), (32, 255), (128, 246), (128, 247)}
    for c in cs:
        if c.family == "bwd":
            p = c.data(torch.float16)[0][0]
            assert p.b.Wq == 2 * P.slab_rows(p.a, p.b) + 3 and p.a.tdx[0] > 0 and p.b.flags & G.EPI_ACCUM and p.b.R == p.a.A
            if c.feat["maskbits"]:
                assert p.a.ldxb == p.b.N // 8 + 4 and p.a.flags & G.EPI_MASKBITS and p.b.flags & G.EPI_MASKBITS
            else:
                x = c.data(torch.float16)[1][p.a.X].data
                assert ((x == 0) & torch.signbit(x)).any() and ((x != 0) & (x.abs() < torch.finfo(torch.float16).smallest_normal)).any()
    assert {(c.feat["C"], c.feat["T"]) for c in cs if c.family == "single"} == {(C, T) for C in P.WIDTHS for T in (255, 256, 257)}
    halos = {sum(P.halo(c.data(torch.float16)[0][0].b)) for c in cs if c.family == "taps"}
    assert halos == {0, 1, 4, 45}
    g3 = P.BY_NAME["group3-c64"].data(torch.float16)[0]
    assert [p.b.ntaps for p in g3] == [3, 11, 7] and [(p.b.M // p.b.Wq, p.b.Wq) for p in g3] == [(2, 300), (1, 520), (3, 100)]
    gs = P.BY_NAME["group-same-c-c64"].data(torch.float16)[0]
    assert gs[0].b.C == gs[1].b.C and gs[0].b.C2 != gs[1].b.C2
    dead = [c for c in cs if c.family == "dead" and "skipped" in c.feat]
    assert sorted(c.feat["skipped"] for c in dead if c.feat["C"] == 64 and "fwd" in c.name) == [0, 0, 1, 1, 2]
    assert {c.feat["C"] for c in dead} == set(P.WIDTHS)
    gd = P.BY_NAME["dead-group-c64"].data(torch.float16)[0]
    assert len({p.dead for p in gd}) == 3


def _ratios(outs, got, adt, extra_rnd=None):
    """extra_rnd: {name: flat roundings that are as unavoidable as the output's own} (a second launch that accumulates onto the first's
    16-bit result inherits that result's rounding)"""
    worst = share = 0.0
    for name, (val, bd, cnt) in outs.items():
        w = cnt > 0
        if not w.any():
            continue
        err, ref = (got[name][w] - val[w]).abs(), val[w].abs()
        assert torch.isfinite(got[name][w]).all()
        worst = max(worst, (err / bd[w]).max().item())
        rnd = G.act_eps(adt) * ref + G.act_tiny(adt) / 2
        if extra_rnd and name in extra_rnd:
            rnd = rnd + extra_rnd[name][w]
        share = max(share, ((err - rnd) / (bd[w] - rnd)).max().item())
    return worst, share


@pytest.mark.parametrize("adt", ADTS, ids=IDS)
@pytest.mark.parametrize("name", NAMES)
def test_emulated_pair_stays_inside_half_the_bound(name, adt):
    case = P.BY_NAME[name]
    problems, bufs, _ = case.data(adt)
    outs, bits = case.expected(adt)
    src = P.bits_source(problems)
    extra = None
    if case.feat.get("sequential"):                         # two launches, two roundings: the first result's rounding reaches the second's outputs
        v1 = P.expected_pair(problems[:1], bufs, adt)[0][problems[0].b.C][0]
        r1 = G.act_eps(adt) * v1.abs() + G.act_tiny(adt) / 2
        extra = {problems[1].b.C: r1, problems[1].b.C2: r1}
    for order in ("seq", "blk32"):
        got = P.emulate_pair(problems, bufs, adt, order)
        worst, share = _ratios(outs, got, adt, extra)
        print(f"{name} {adt} {order}: emulated err / bound = {worst:.3f}, share beside the output rounding = {share:.3f}")
        assert share <= 0.5, (order, share)
        assert worst <= 1.0
        for bname, eb in bits.items():
            st = src[bname]
            assert G.check_bits(bname, got[bname], eb, st, got[st[0]] if st else None) == 0, bname
        for nm in got:                                      # skipped slabs and pad bytes keep their contents
            cnt = outs[nm][2] if nm in outs else bits[nm][2] if nm in bits else torch.zeros(got[nm].numel(), dtype=torch.int64)
            a, b = got[nm][cnt == 0], bufs[nm].data[cnt == 0]
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)), nm
        if case.feat.get("sharp"):                          # the sharp reference: stage b on the (emulated) stored tape, plain bound
            stored = {p.a.C2: got[p.a.C2] for p in problems if p.a is not None and p.a.C2 is not None}
            souts, _ = P.expected_pair(problems, bufs, adt, stored=stored)
            for k in stored:
                souts.pop(k)
            sworst, sshare = _ratios(souts, got, adt)
            print(f"{name} {adt} {order}: sharp err / bound = {sworst:.3f}, share = {sshare:.3f}, sharp_fraction = {P.sharp_fraction(souts, bufs, adt):.3f}")
            assert sshare <= 0.5 and sworst <= 1.0
    print(f"{name} {adt}: sharp_fraction (universal bound) = {P.sharp_fraction(outs, bufs, adt):.3f}")


@pytest.mark.parametrize("adt", ADTS, ids=IDS)
@pytest.mark.parametrize("name", NAMES)
def test_every_applicable_pair_mutant_leaves_the_bound(name, adt):
    case = P.BY_NAME[name]
    problems, bufs, _ = case.data(adt)
    outs, bits = case.expected(adt)
    weakest = None
    for mut, applies in P.MUTANTS.items():
        if not applies(case):
            continue
        mo, mb = P.expected_pair(problems, bufs, adt, mut)
        ratio = G.mutant_ratio(outs, mo, bits, mb)
        print(f"{name} {adt}: mutant {mut} err / bound = {ratio:.3g}")
        weakest = ratio if weakest is None else min(weakest, ratio)
        assert ratio > 1.0, (mut, ratio)
    assert weakest is not None
    print(f"{name} {adt}: weakest mutant ratio = {weakest:.3g}")


def test_each_pair_mutant_is_applied_somewhere():
    for mut, applies in P.MUTANTS.items():
        assert any(applies(c) for c in P.CASES), mut


@pytest.mark.parametrize("adt", ADTS, ids=IDS)
def test_ambiguous_signs_of_a_bits_only_tape_are_rare(adt):
    """from the reference alone: the free bits are at most 1 % of the intermediate in every case that compares bits only"""
    seen = 0
    for c in P.CASES:
        if not c.feat.get("bits_only"):
            continue
        problems, _, _ = c.data(adt)
        _, bits = c.expected(adt)
        for p in problems:
            ref, free, cnt = bits[p.a.B2]
            w = cnt > 0
            nfree = sum(bin(int(v)).count("1") for v in free[w].tolist())
            share = nfree / (8 * int(w.sum()))
            print(f"{c.name} {adt}: ambiguous-sign share = {share:.2e}")
            assert share <= 0.01, (c.name, share)
            seen += 1
    assert seen >= 6
