"""-m gpu: the implicit-GEMM kernel family and its epilogues (csrc/gemm_tile.h, gemm_conv.hip, gemm_ln.hip, gemm_epilogue.h, the split-K
reduce kernel) through the C-ABI test hook dmx_gemm_raw, ELEMENT BY ELEMENT against the float64 model of tests/gemm_cases.py on the same
16-bit-rounded operands.  Every output buffer is pre-filled with a sentinel bit pattern; a case passes when
  - every element the launches may write is finite and within the element-wise bound of the reference (C and C2), and
  - every other element -- pad columns >= N of a wider buffer, rows >= M, C under EPI_NO_C, columns >= N / 2 under EPI_GEGLU, the rows of
    the other phases of a multi-launch operator -- still holds its sentinel, bit for bit, and
  - every sign byte of an EPI_BITS2 launch equals the sign bits of the 16-bit values the launch itself stored.
The bound comes from the number formats (gemm_cases docstring; tests/test_gemm_bound_host.py validates it without a GPU); each case
prints its observed err / bound and where it sits.

Observed on an MI355X (fp16 build), largest err / bound per family -- recorded, never fed back into a bound.  Every case passed on
its first run; neither the model nor a kernel had to change:
    tile-bias-rowbias-resid 0.649   tile-mask-resid-accum 0.657   tile-bias-residinv-lrelu2 0.655   ...-noc 0.655   tile-tanh 0.627
    direct 0.634   mtail 0.583   batched 0.643   rowmap 0.659   geglu 0.997   geglu-ln 0.965   geglu-exact 0.999   softbwd 0.990
    bits (EPI_MASKBITS / EPI_BITS2, N = 8 / 16 / 88 on tiles 0 / 6 / 12) 0.651, 0 wrong sign bytes
    splitk (plans 212 / 313 and the unsplit tile 12) 0.585, with EPI_NO_C 0.569"""
import ctypes as C

import pytest
import torch

from tests import gemm_cases as G

pytestmark = pytest.mark.gpu


def _L():
    from diffmusic_amd import _lib as L
    return L


def _adt():
    return _L().act_dtype()


def _upload(buf, adt):
    """flat float64 buffer -> device tensor of raw bits (int16 / int32), sentinel bits where the buffer holds NaN"""
    nan = torch.isnan(buf.data)
    v = torch.nan_to_num(buf.data, nan=0.0)
    if buf.kind == "bits":
        bits = v.to(torch.uint8)
        bits[nan] = G.SENT8
    elif buf.kind == "act":
        bits = v.to(adt).view(torch.int16).clone()
        bits[nan] = G.SENT16
    else:
        bits = v.float().view(torch.int32).clone()
        bits[nan] = G.SENT32
    return bits.cuda()


def _values(bits, kind, adt):
    return (bits.view(adt) if kind == "act" else bits.view(torch.float32)).double()


def _desc(L, ln, dev):
    d = L.GemmDesc()
    for k in G.INT_FIELDS:
        setattr(d, k, getattr(ln, k))
    for k in G.FLOAT_FIELDS:
        setattr(d, k, getattr(ln, k))
    for k in G.PTR_FIELDS:
        name = getattr(ln, k)
        setattr(d, k, dev[name].data_ptr() if name is not None else None)
    for i in range(ln.ntaps):
        d.tdy[i], d.tdx[i] = ln.tdy[i], ln.tdx[i]
    return d


def _raw(L, d):
    return L.lib().dmx_gemm_raw(C.byref(d), C.sizeof(d), C.c_void_p(torch.cuda.current_stream().cuda_stream))


class _splitk_scratch:
    """the split-K workspace a forced plan needs, released on the way out"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            L = _L()
            self.ws = torch.empty(1 << 18, dtype=torch.float32, device="cuda")
            L.check(L.lib().dmx_gemm_splitk_workspace(C.c_void_p(self.ws.data_ptr()), self.ws.numel() * 4), "ws")

    def __exit__(self, *exc):
        if self.on:
            torch.cuda.synchronize()
            _L().lib().dmx_gemm_splitk_workspace(None, 0)


def _run_case(case):
    """-> {output name: bits on the CPU} after running every launch of the case"""
    L, adt = _L(), _adt()
    launches, bufs, _ = case.data(adt)
    dev = {k: _upload(b, adt) for k, b in bufs.items()}
    with _splitk_scratch(case.tile >= 100):
        for ln in launches:
            L.check(_raw(L, _desc(L, ln, dev)), case.name)
        torch.cuda.synchronize()
    return {k: dev[k].cpu() for ln in launches for k in (ln.C, ln.C2, ln.B2) if k is not None}


def _check(case, out):
    """asserts the case; -> the largest err / bound"""
    adt = _adt()
    bufs = case.data(adt)[1]
    worst, where = 0.0, None
    for name, (val, bd, cnt) in case.expected(adt).items():
        kind = bufs[name].kind
        w = cnt > 0
        bits = out[name]
        sent = G.SENT16 if kind == "act" else G.SENT32
        touched = (bits[~w] != sent).nonzero().flatten()
        assert touched.numel() == 0, f"{case.name}: {name} written outside the writable set, first at flat index {(~w).nonzero().flatten()[touched[0]].item()}"
        if not w.any():
            continue
        got = _values(bits, kind, adt)[w]
        assert torch.isfinite(got).all(), f"{case.name}: {name} holds non-finite values"
        ratio = (got - val[w]).abs() / bd[w]
        i = int(ratio.argmax())
        if (ratio > 1.0).any():
            ldn = getattr(case.data(adt)[0][0], "ldc" if name == "C" else "ldc2")
            flat = w.nonzero().flatten()[(ratio > 1.0).nonzero().flatten()]
            print(f"{case.name}: {name} has {flat.numel()} elements outside the bound, first at (row, col) "
                  + ", ".join(f"({int(f) // ldn}, {int(f) % ldn})" for f in flat[:12]))
        if ratio[i].item() >= worst:
            ld = getattr(case.data(adt)[0][0], "ldc" if name == "C" else "ldc2")
            flat = int(w.nonzero().flatten()[i])
            worst, where = ratio[i].item(), f"{name}[row {flat // ld}, col {flat % ld}] got {got[i].item():.6g} ref {val[w][i].item():.6g}"
    src = G.bits_source(case.data(adt)[0])
    for name, eb in case.expected_bits(adt).items():       # EPI_BITS2: the third kind of write, compared exactly
        got = out[name]
        assert (got[eb[2] == 0] == G.SENT8).all(), f"{case.name}: {name} written outside the writable set"
        st = src[name]
        bad = G.check_bits(name, got, eb, st, _values(out[st[0]], "act", adt) if st else None)
        print(f"{case.name}: {name} wrong sign bytes = {bad} of {int((eb[2] > 0).sum())}")
        assert bad == 0, (case.name, name, bad)
    print(f"{case.name}: max err / bound = {worst:.3f} at {where}")
    assert worst <= 1.0, (case.name, worst, where)
    return worst


@pytest.mark.parametrize("name", [c.name for c in G.CASES if c.family != "splitk"])
def test_gemm_epilogue_elementwise(name):
    case = G.BY_NAME[name]
    _check(case, _run_case(case))


@pytest.mark.parametrize("tag", ["", "-noc"])
@pytest.mark.parametrize("plan", [212, 313])
def test_forced_split_k_plan_elementwise(plan, tag):
    """the reduce kernel's epilogue (mask, bias, row bias, inverse-slope residual, alpha, leaky-relu second output, EPI_NO_C) against the
    reference, and against the unsplit tile 12 on the same operands"""
    split, single = G.BY_NAME[f"splitk{tag}-{plan}"], G.BY_NAME[f"splitk{tag}-12"]
    o_split, o_single = _run_case(split), _run_case(single)
    _check(split, o_split)
    _check(single, o_single)
    adt = _adt()
    for name, (val, bd, cnt) in split.expected(adt).items():
        w = cnt > 0
        if w.any():
            a, b = _values(o_split[name], "act", adt)[w], _values(o_single[name], "act", adt)[w]
            assert ((a - b).abs() <= 2 * bd[w]).all(), name


def _geglu_refusal_variants():
    def resid(ln, dev):
        ln.flags |= G.EPI_RESID
        ln.R, ln.ldr = "C", ln.ldc

    def n_tail(ln, dev):
        ln.N -= 16

    def narrow_ldc(ln, dev):
        ln.ldc = ln.N // 2 - 8

    def alpha(ln, dev):
        ln.alpha = 0.5

    def row_map(ln, dev):
        ln.osx, ln.Wo = 2, 2 * ln.M

    def odd_side_stride(ln, dev):                       # would take the direct epilogue, which knows no GEGLU
        ln.ldr = 4
    return {"resid": resid, "n-not-32": n_tail, "ldc-below-half": narrow_ldc, "alpha": alpha, "row-map": row_map, "ldr-not-8": odd_side_stride}


@pytest.mark.parametrize("what", list(_geglu_refusal_variants()))
def test_geglu_refusals(what):
    """descriptors the fused GEGLU does not take are refused ahead of any launch: non-zero return, output untouched"""
    from types import SimpleNamespace
    L, adt = _L(), _adt()
    launches, bufs, _ = G.BY_NAME["geglu-tile6"].data(adt)
    ln = SimpleNamespace(**vars(launches[0]))
    dev = {k: _upload(b, adt) for k, b in bufs.items()}
    _geglu_refusal_variants()[what](ln, dev)
    ln.K = ln.ntaps * ln.Ci
    assert _raw(L, _desc(L, ln, dev)) != 0, what
    torch.cuda.synchronize()
    assert (dev["C"] == G.SENT16).all()


def test_forced_split_k_plan_with_tanh_is_refused():
    L, adt = _L(), _adt()
    from types import SimpleNamespace
    launches, bufs, _ = G.BY_NAME["splitk-212"].data(adt)
    ln = SimpleNamespace(**vars(launches[0]))
    ln.flags = G.EPI_TANH
    dev = {k: _upload(b, adt) for k, b in bufs.items()}
    with _splitk_scratch(True):
        assert _raw(L, _desc(L, ln, dev)) != 0
        torch.cuda.synchronize()
    assert (dev["C"] == G.SENT16).all() and (dev["C2"] == G.SENT16).all()
