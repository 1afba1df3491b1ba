"""CPU: the float64 model, the element-wise bound and the case table of tests/gemm_cases.py are validated from the reference alone, for
both activation types, so that the tolerance of tests/test_gpu_gemm_elementwise.py is never fitted to a kernel:
  - the model of GemmDesc agrees with torch's own float64 conv1d / conv_transpose1d / conv2d / interpolate + conv2d / autograd /
    layer_norm / gelu on every descriptor builder: the descriptors under test are the operations the models run;
  - an fp32 emulation of the kernels' arithmetic (two accumulation orders, bias-first start, split-K slices, the fp32 epilogue, the
    LayerNorm fold's slot sums and fma, one rounding to the output type) stays inside half the bound -- for 16-bit outputs half of
    what the bound leaves beside the one unavoidable output rounding (gemm_cases docstring);
  - every applicable mutant of the reference leaves the bound in every case that exercises what it breaks, and applies somewhere;
  - the K <= 72 cases are sharp; the table covers tiles 1 .. 19 and every flag."""
import pytest
import torch

from tests import gemm_cases as G

ADTS = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
NAMES = [c.name for c in G.CASES]


def test_flag_values_are_the_bindings():
    from diffmusic_amd import _lib as L
    for name, v in G.FLAG_NAMES.items():
        assert getattr(L, "EPI_" + name) == v, name


def _logical(launches, bufs, name="C"):
    """the written region of an output as (rows, columns), NaN where no launch wrote; asserts the pad columns kept their sentinel"""
    L = launches[0]
    val, _, cnt = G.expected(launches, bufs, None)[name]
    ld = L.ldc if name == "C" else L.ldc2
    ncol = L.N // 2 if L.flags & G.EPI_GEGLU else L.N
    v, c = val.view(-1, ld), cnt.view(-1, ld)
    assert torch.isnan(v[:, ncol:]).all() and (c[:, ncol:] == 0).all()
    return v[:, :ncol], c[:, :ncol]


BUILDERS = {
    "conv1d": lambda: G.conv1d_case("b-conv1d", 2, 41, 16, 24, 5, 3, 0),
    "convT-s4": lambda: G.convT1d_case("b-convT4", 2, 37, 16, 24, 8, 4, 2, 0),
    "convT-s5": lambda: G.convT1d_case("b-convT5", 2, 37, 16, 24, 11, 5, 3, 0),
    "convT-s4-dgrad": lambda: G.convT1d_dgrad_case("b-convT4d", 2, 37, 16, 24, 8, 4, 2),
    "convT-s5-dgrad": lambda: G.convT1d_dgrad_case("b-convT5d", 2, 37, 16, 24, 11, 5, 3),
    "conv2d-s2": lambda: G.conv2d_s2_case("b-c2s2", 2, 9, 11, 16, 24, 0),
    "up2x-fwd": lambda: G.up2x_fwd_case("b-upf", 2, 5, 7, 16, 24, 0),
    "up2x-bwd": lambda: G.up2x_bwd_case("b-upb", 2, 5, 7, 16, 24),
    "conv2d-3x3": lambda: G.conv2d_3x3_case("b-c33", 2, 5, 5, 16, 24, 0),
    "gemm-nt": lambda: G.gemm_nt_case("b-nt", 1, 1, 37, 24, 40, 0),
    "gemm-nt-batched": lambda: G.gemm_nt_case("b-ntz", 6, 3, 19, 24, 40, 0),
    "softbwd": lambda: G.softbwd_case("b-soft", 2, 40, 24),
    "geglu": lambda: G.geglu_case("b-geglu", 37, 40, 96, 0),
    "geglu-ln": lambda: G.geglu_case("b-geglu-ln", 37, 72, 96, 0, ln=True),
}


@pytest.mark.parametrize("which", list(BUILDERS))
def test_model_of_the_descriptor_is_the_torch_operation(which):
    launches, bufs, tref = BUILDERS[which]()
    for L in launches:
        G.finish_ln(bufs, L)
    got, cnt = _logical(launches, bufs)
    want = tref(bufs)
    assert got.shape == want.shape
    assert (cnt == 1).all(), "every output element is written exactly once by the union of the launches"
    err = (got - want).abs().max().item()
    print(f"{which}: max |model - torch float64| = {err:.2e}")
    assert err < 1e-11 * max(1.0, want.abs().max().item())


def test_epilogue_order_against_plain_torch():
    """the documented order on one descriptor with every pointwise flag: mask -> bias -> rowbias -> residual (inverse slope) -> alpha ->
    accum -> C, leaky-relu -> C2"""
    fl = G.EPI_BIAS | G.EPI_ROWBIAS | G.EPI_MASK | G.EPI_RESID | G.EPI_RESID_INV | G.EPI_ACCUM | G.EPI_LRELU2
    launches, bufs, tref = G.conv1d_case("b-epi", 3, 20, 8, 16, 3, 1, fl, alpha=0.5, ld_pad=8)
    L = launches[0]
    prev = bufs["C"].data.view(-1, L.ldc)[:, :16].clone()
    c, _ = _logical(launches, bufs)
    c2, _ = _logical(launches, bufs, "C2")
    x, r = bufs["X"].data.view(-1, L.ldx)[:, :16], bufs["R"].data.view(-1, L.ldr)[:, :16]
    rb = bufs["rowbias"].data.view(3, L.ldrb)[:, :16].repeat_interleave(20, 0)
    v = tref(bufs) * torch.where(x > 0, 1.0, 0.1) + bufs["bias"].data + rb + torch.where(r > 0, r, r * 10.0)
    v = v * 0.5 + prev
    assert (c - v).abs().max().item() < 1e-12 and (c2 - torch.nn.functional.leaky_relu(v, 0.1)).abs().max().item() < 1e-12
    launches, bufs, tref = G.conv1d_case("b-tanh", 3, 20, 8, 16, 3, 1, G.EPI_BIAS | G.EPI_TANH | G.EPI_F32OUT, kind="f32")
    c, _ = _logical(launches, bufs)
    assert (c - torch.tanh(tref(bufs) + bufs["bias"].data)).abs().max().item() < 1e-12


def test_case_table_covers_tiles_flags_and_edges():
    cs = G.CASES
    for f in G.FLAG_SETS:
        assert {c.tile for c in cs if c.family == "tile-" + f} == set(range(1, 20)), f
    for c in cs:
        if c.family.startswith("tile-"):
            BM, BN = G.TILES[c.tile]
            L = c.data(torch.float16)[0][0]
            assert (L.M, L.N, L.K) == (BM + 17, BN + 24, 72) and L.ldc == L.ldr == L.ldx == L.ldc2 == L.N + 8 and L.Hq * L.Wq == 50
            assert L.N % 8 == 0                         # the LDS-staged epilogue
    for name, v in G.FLAG_NAMES.items():
        assert any(c.flags & v for c in cs), name
    f1 = G.BY_NAME["tile7-bias-rowbias-resid"].data(torch.float16)[0][0]
    assert f1.alpha == 0.5 and f1.ldrb == f1.N + 4
    x = G.BY_NAME["tile1-mask-resid-accum"].data(torch.float16)[1]["X"].data
    assert ((x == 0) & ~torch.signbit(x)).any() and ((x == 0) & torch.signbit(x)).any()
    assert ((x != 0) & (x.abs() < torch.finfo(torch.float16).smallest_normal)).any()
    d = [c for c in cs if c.family == "direct"]
    assert {c.feat["N"] for c in d} == {8, 12} and any(c.flags & G.EPI_F32OUT and c.flags & G.EPI_TANH and c.flags & G.EPI_BIAS for c in d)
    assert any(c.flags & G.EPI_F32OUT and c.flags & G.EPI_ACCUM for c in d)
    assert any(not c.flags & G.EPI_F32OUT and c.flags & G.EPI_ACCUM and c.flags & G.EPI_ROWBIAS and c.flags & G.EPI_LRELU2 for c in d)
    assert {c.tile for c in cs if c.family == "mtail"} == {6, 12} and all(c.feat["M"] == 5 for c in cs if c.family == "mtail")
    assert all(c.feat["Z"] == 4 and c.feat["N"] == 136 for c in cs if c.family == "batched")
    assert {c.tile for c in cs if c.family == "geglu" and c.feat["N"] != 96 or c.family == "geglu" and G.TILES[c.tile][1] == 64} \
        == {3, 4, 5, 6} | set(G.DMA_TILES)
    assert any(c.family == "geglu" and c.feat["N"] == 96 for c in cs)
    assert [c.tile for c in cs if c.family == "geglu-ln"] == G.LN_TILES
    assert {c.tile for c in cs if c.family == "splitk"} == {12, 212, 313}
    bits = [c for c in cs if c.family == "bits"]
    assert {(c.feat["N"], c.tile) for c in bits} == {(N, t) for N in (8, 16, 88) for t in (0, 6, 12)}
    for c in bits:
        L = c.data(torch.float16)[0][0]
        assert (L.Ci, L.ntaps, L.Hq * L.Wq) == (24, 3, 50)
        if c.flags & G.EPI_MASKBITS:
            assert L.ldxb > L.N // 8 and c.flags & G.EPI_RESID
        if c.flags & G.EPI_BITS2:
            assert L.ldb2 > L.N // 8 and c.flags & G.EPI_LRELU2
    assert any(c.flags & G.EPI_BITS2 and c.flags & G.EPI_NO_C for c in bits) and any(c.flags & G.EPI_BITS2 and not c.flags & G.EPI_NO_C for c in bits)
    for c in cs:
        if c.family == "rowmap" and c.feat.get("multi"):
            for val, bd, cnt in c.expected(torch.float16).values():
                assert (cnt.view(-1, c.data(torch.float16)[0][0].ldc)[:, :24] == 1).all(), c.name      # the phases tile the output exactly
    # the LayerNorm-fold rows keep |mean| <= std, the GEGLU gates reach +-10
    L, bufs, _ = G.BY_NAME["geglu-ln-tile12"].data(torch.float16)
    x = bufs["A"].data.view(L[0].M, L[0].K)
    assert (x.mean(1).abs() <= x.std(1)).all()
    L, bufs, _ = G.BY_NAME["geglu-tile12"].data(torch.float16)
    acc = bufs["A"].data.view(L[0].M, 72) @ bufs["W"].data.view(L[0].N, 72).t()
    g = acc[:, G.geglu_cols(L[0].N) + 16]
    assert g.max() > 10 and g.min() < -10
    L, bufs, _ = G.BY_NAME["geglu-exact-gate-tile6"].data(torch.float16)
    Ag, Wm = G.gather(L[0], bufs, 0)
    assert torch.equal((Ag @ Wm.t())[:, G.geglu_cols(96) + 16], Ag[:, :1].expand(-1, 48))              # the gate accumulators are column 0, exactly


def _ratios(case, adt, got):
    """(largest err / bound, largest share of what the bound leaves beside one output rounding) over the written elements"""
    worst = share = 0.0
    for name, (val, bd, cnt) in case.expected(adt).items():
        w = cnt > 0
        if not w.any():                                 # (C under EPI_NO_C)
            continue
        err, ref = (got[name][w] - val[w]).abs(), val[w].abs()
        assert torch.isfinite(got[name][w]).all()
        worst = max(worst, (err / bd[w]).max().item())
        if case.data(adt)[1][name].kind == "f32":
            share = max(share, (err / bd[w]).max().item())
        else:
            rnd = G.act_eps(adt) * ref + G.act_tiny(adt) / 2
            share = max(share, ((err - rnd) / (bd[w] - rnd)).max().item())
    return worst, share


def _bits_ok(case, adt, got):
    """the sign bytes of an emulated run: exact against what it stored, or against the reference outside the free bits"""
    src = G.bits_source(case.data(adt)[0])
    for name, eb in case.expected_bits(adt).items():
        bad = G.check_bits(name, got[name], eb, src[name], got[src[name][0]] if src[name] else None)
        assert bad == 0, (case.name, name, bad)
        assert torch.isnan(got[name][eb[2] == 0]).all()


@pytest.mark.parametrize("adt", ADTS, ids=IDS)
@pytest.mark.parametrize("name", NAMES)
def test_emulated_kernel_stays_inside_half_the_bound(name, adt):
    case = G.BY_NAME[name]
    launches, bufs, _ = case.data(adt)
    for order in ("seq", "blk32"):
        got = G.emulate(launches, bufs, adt, order)
        _bits_ok(case, adt, got)
        worst, share = _ratios(case, adt, got)
        print(f"{name} {adt} {order}: emulated err / bound = {worst:.3f}, share beside the output rounding = {share:.3f}")
        assert share <= 0.5, (order, share)
        assert worst <= 1.0


@pytest.mark.parametrize("adt", ADTS, ids=IDS)
@pytest.mark.parametrize("name", NAMES)
def test_every_applicable_mutant_leaves_the_bound(name, adt):
    case = G.BY_NAME[name]
    exp = case.expected(adt)
    launches, bufs, _ = case.data(adt)
    applied = []
    for mut, applies in G.MUTANTS.items():
        if not applies(case):
            continue
        mo, mb = G.expected_all(launches, bufs, adt, mut)
        ratio = G.mutant_ratio(exp, mo, case.expected_bits(adt), mb)
        print(f"{name} {adt}: mutant {mut} err / bound = {ratio:.3g}")
        applied.append(mut)
        assert ratio > 1.0, (mut, ratio)
    assert applied


def test_each_mutant_is_applied_somewhere():
    for mut, applies in G.MUTANTS.items():
        assert any(applies(c) for c in G.CASES), mut


@pytest.mark.parametrize("adt", ADTS, ids=IDS)
def test_shallow_cases_are_sharp(adt):
    """K <= 72: the accumulation term exceeds the output term in at most 10 % of the elements"""
    worst = {}
    for c in G.CASES:
        L = c.data(adt)[0]
        if max(l.K for l in L) > 72:
            continue
        fr = G.sharp_fraction(c, adt)
        worst[c.family] = max(worst.get(c.family, 0.0), fr)
        assert fr <= 0.10, (c.name, fr)
    print(f"{adt}: largest share of elements with accumulation term > output term, per family: "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
