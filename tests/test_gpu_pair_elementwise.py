"""-m gpu: the fused convolution pair (csrc/conv_pair.hip) through the C-ABI test hooks dmx_conv_pair_raw / dmx_conv_pair_group_raw /
dmx_conv_pair_dead_raw / dmx_conv_pair_group_dead_raw, ELEMENT BY ELEMENT against the two-stage float64 model of tests/pair_cases.py on the
same 16-bit-rounded operands.  It works like tests/test_gpu_gemm_elementwise.py: every output and tape buffer is pre-filled with its
sentinel; a case passes when
  - every element the launch may write is finite and within its element-wise bound (the universal bound of pair_cases, from the number
    formats only),
  - where the tape tensor a.C2 is stored, stage b is also within the PLAIN single-launch bound of the model run on the stored a.C2 bits
    (the sharp check),
  - every sign byte equals the sign bits of the stored tape tensor, or -- bits-only tapes -- the reference outside the ambiguous set, and
  - every other byte of EVERY buffer of the case, inputs included, is what it was before the launch (skipped slabs, EPI_NO_C targets, pad
    bytes of wider rows, the never-written a.C).
Each case prints its observed err / bound (tests/test_pair_bound_host.py validates the bound without a GPU).

Observed on an MI355X (fp16 build), largest err / bound per family, universal / sharp -- recorded, never fed back into a bound:
    forward grid      C = 32: 0.621 / 0.650   C = 64: 0.584 / 0.637   C = 128: 0.507 / 0.611
    forward variants  C = 32: 0.630 / 0.652   C = 64: 0.500 / 0.604   C = 128: 0.262 / 0.493
    T edges           C = 32: 0.621 / 0.642   C = 64: 0.560 / 0.602   C = 128: 0.261 / 0.496
    unused tap shapes C = 32: 0.650 / 0.660   C = 64: 0.637 / 0.653   (k = 1, k = 2, causal, k = 16 dil 3: all right, none refused)
    backward + twins  C = 32: 0.599           C = 64: 0.556           C = 128: 0.483          (twins bit for bit)
    single stage      C = 32: 0.594           C = 64: 0.532           C = 128: 0.427
    grouped           C = 32: 0.623           C = 64: 0.591           C = 128: 0.528          (bit for bit the separate launches)
    dead rows         C = 32: 0.572           C = 64: 0.572           C = 128: 0.370
    sign bytes: 0 wrong in every case, stored tapes and bits-only tapes alike.
No case exposed a fault of the kernel; the one change the work forced is the refusal of sign-bit mask rows that do not start on a
32-bit word (ldxb % 4 != 0), which the kernel loads as words."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

from tests import gemm_cases as G
from tests import pair_cases as P
from tests.test_gpu_gemm_elementwise import _L, _adt, _desc, _upload, _values

pytestmark = pytest.mark.gpu
NAN16 = 0x7FFF                           # a NaN in fp16 and in bf16


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _upload_case(case, bufs, adt):
    dev = {k: _upload(b, adt) for k, b in bufs.items()}
    if "nan_rows" in case.feat:                             # rows the launch must read as zeros hold NaNs in memory
        p = case.data(adt)[0][0]
        z0, z1 = case.feat["zero"]
        T, Cc = p.b.Wq, p.b.N
        dev[case.feat["nan_rows"]].view(-1, T, Cc)[:, z0:z1] = NAN16
    return dev


def _launch(case, problems, dev, how):
    """-> (return code, (skipped, total) or None)"""
    L = _L()
    lib = L.lib()
    n = len(problems)
    if how in ("pair", "dead"):
        assert n == 1
        p = problems[0]
        da = _desc(L, p.a, dev) if p.a is not None else None
        db = _desc(L, p.b, dev)
        pa = C.byref(da) if da is not None else None
        if how == "pair":
            return lib.dmx_conv_pair_raw(pa, C.byref(db), C.sizeof(db), _stream()), None
        dead = (C.c_int * 4)(*p.dead) if p.dead is not None else None
        sk, tot = C.c_int(-1), C.c_int(-1)
        rc = lib.dmx_conv_pair_dead_raw(pa, C.byref(db), C.sizeof(db), dead, C.byref(sk), C.byref(tot), _stream())
        return rc, (sk.value, tot.value)
    das, dbs = (L.GemmDesc * n)(), (L.GemmDesc * n)()
    for j, p in enumerate(problems):
        das[j], dbs[j] = _desc(L, p.a, dev), _desc(L, p.b, dev)
    if how == "group":
        return lib.dmx_conv_pair_group_raw(n, C.byref(das), C.byref(dbs), C.sizeof(L.GemmDesc), _stream()), None
    dead = (C.c_int * (4 * n))(*[v for p in problems for v in (p.dead or (0, 0, 0, 0))])
    return lib.dmx_conv_pair_group_dead_raw(n, C.byref(das), C.byref(dbs), C.sizeof(L.GemmDesc), dead, _stream()), None


def _run(case, how=None, one_by_one=False):
    """-> (buffers after the launch, buffers before it, (skipped, total) or None), all on the CPU as raw bits"""
    L, adt = _L(), _adt()
    problems, bufs, _ = case.data(adt)
    dev = _upload_case(case, bufs, adt)
    init = {k: v.cpu().clone() for k, v in dev.items()}
    info = None
    if one_by_one:
        for p in problems:
            rc, _ = _launch(case, [p], dev, "dead" if p.dead is not None else "pair")
            L.check(rc, case.name)
    else:
        rc, info = _launch(case, problems, dev, how or case.how)
        L.check(rc, case.name)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dev.items()}, init, info


def _within(case, out, outs, bufs, adt, what):
    """every written element finite and within its bound; -> largest err / bound"""
    worst, where = 0.0, None
    for name, (val, bd, cnt) in outs.items():
        w = cnt > 0
        if not w.any():
            continue
        got = _values(out[name], "act", adt)[w]
        assert torch.isfinite(got).all(), f"{case.name}: {name} holds non-finite values"
        ratio = (got - val[w]).abs() / bd[w]
        bad = int((ratio > 1.0).sum())
        i = int(ratio.argmax())
        if bad:
            ld = case.data(adt)[0][0].b.N
            flat = w.nonzero().flatten()[(ratio > 1.0).nonzero().flatten()[:8]]
            print(f"{case.name} {what}: {name} has {bad} of {int(w.sum())} elements outside the bound, first at (row, col) "
                  + ", ".join(f"({int(f) // ld}, {int(f) % ld})" for f in flat))
        if ratio[i].item() >= worst:
            flat = int(w.nonzero().flatten()[i])
            worst, where = ratio[i].item(), f"{name}[flat {flat}] got {got[i].item():.6g} ref {val[w][i].item():.6g}"
    print(f"{case.name} {what}: max err / bound = {worst:.3f} at {where}")
    return worst


def _check(case, out, init):
    """asserts the case; -> (largest universal err / bound, largest sharp err / bound or None)"""
    adt = _adt()
    problems, bufs, _ = case.data(adt)
    outs, bits = case.expected(adt)
    # ---- nothing outside the writable set changed, in any buffer of the case
    for name in out:
        cnt = outs[name][2] if name in outs else bits[name][2] if name in bits else None
        same = out[name] == init[name]
        untouched = same if cnt is None else same[cnt == 0]
        assert untouched.all(), f"{case.name}: {name} changed outside the writable set ({int((~untouched).sum())} elements)"
    worst = _within(case, out, outs, bufs, adt, "universal")
    # ---- sign bytes, exactly
    src = P.bits_source(problems)
    for name, eb in bits.items():
        st = src[name]
        bad = G.check_bits(name, out[name], eb, st, _values(out[st[0]], "act", adt) if st else None)
        print(f"{case.name}: {name} wrong sign bytes = {bad} of {int((eb[2] > 0).sum())}" + ("" if st else " (bits only: against the reference)"))
        assert bad == 0, (case.name, name, bad)
    assert worst <= 1.0, (case.name, worst)
    # ---- sharp: stage b against the model run on the tape tensor the kernel stored
    sharp = None
    if case.feat.get("sharp"):
        stored = {p.a.C2: _values(out[p.a.C2], "act", adt) for p in problems if p.a is not None and p.a.C2 is not None}
        souts, _ = P.expected_pair(problems, bufs, adt, stored=stored)
        for k in stored:                                    # (the tape itself was held against h above)
            souts.pop(k)
        sharp = _within(case, out, souts, bufs, adt, "sharp")
        assert sharp <= 1.0, (case.name, sharp)
    return worst, sharp


NAMES = [c.name for c in P.CASES if c.family in ("fwd", "fwd-variant", "fwd-edge", "single", "taps")]


@pytest.mark.parametrize("name", NAMES)
def test_pair_elementwise(name):
    case = P.BY_NAME[name]
    out, init, _ = _run(case)
    _check(case, out, init)


@pytest.mark.parametrize("name", [c.name for c in P.CASES if c.family == "bwd" and not c.feat["maskbits"]])
def test_backward_pair_and_its_sign_bit_twin(name):
    """the MASKBITS run is bit for bit the MASK run, and both are within the bound of the reference"""
    case, twin = P.BY_NAME[name], P.BY_NAME[name + "-maskbits"]
    out, init, _ = _run(case)
    _check(case, out, init)
    tout, tinit, _ = _run(twin)
    _check(twin, tout, tinit)
    dst = case.data(_adt())[0][0].b.C
    assert torch.equal(out[dst], tout[dst]), "EPI_MASKBITS and EPI_MASK runs differ"


@pytest.mark.parametrize("name", [c.name for c in P.CASES if c.family == "group"])
def test_grouped_launch_elementwise_and_bitwise_the_separate_launches(name):
    case = P.BY_NAME[name]
    out, init, _ = _run(case)
    _check(case, out, init)
    sep, _, _ = _run(case, one_by_one=True)
    for k in out:
        assert torch.equal(out[k], sep[k]), f"{name}: {k} differs between the grouped launch and separate launches"


@pytest.mark.parametrize("name", [c.name for c in P.CASES if c.family == "dead"])
def test_dead_rows(name):
    """skipped slabs are written nowhere, zero rows count as zeros (they hold NaNs in memory) in the convolution and the slab residual"""
    case = P.BY_NAME[name]
    out, init, info = _run(case)
    if "skipped" in case.feat:
        p = case.data(_adt())[0][0]
        q0, q1 = P.skip_slabs(p.dead, p.b.Wq, P.slab_rows(p.a, p.b))
        assert (q1 - q0, -(-p.b.Wq // P.slab_rows(p.a, p.b))) == (case.feat["skipped"], case.feat["total"])       # the model's count
        assert info == (case.feat["skipped"], case.feat["total"]), info
    _check(case, out, init)
    if case.feat.get("grouped"):
        sep, _, _ = _run(case, one_by_one=True)
        for k in out:
            assert torch.equal(out[k], sep[k]), k


def _refusals():
    """name -> (builder of a base case, mutator of its problem, launch)"""
    fwd = lambda nm, **kw: (lambda: P.forward_case(nm, 2, 100, 64, 7, 3, tape="both", **kw))
    bwd = lambda nm: (lambda: P.backward_case(nm, 2, 100, 64, 7, 3, maskbits=True))

    def set_a(**kw):
        return lambda p: [setattr(p.a, k, v) for k, v in kw.items()]

    def set_b(**kw):
        return lambda p: [setattr(p.b, k, v) for k, v in kw.items()]

    def resid_on_a(p):
        p.a.flags |= G.EPI_RESID
        p.a.R = p.a.A

    def bits2_without_lrelu2(p):
        p.a.flags &= ~G.EPI_LRELU2

    def mask_and_maskbits(p):
        p.a.flags |= G.EPI_MASK
        p.a.X = p.a.A

    def zero_rows(p):
        p.dead = (0, 0, 10, 20)
    return {
        "c48": (lambda: P.forward_case("refuse-c48", 2, 100, 48, 7, 3), None, "pair"),
        "halo52": (lambda: P.forward_case("refuse-halo52", 2, 300, 64, 14, 4), None, "pair"),
        "a-alpha": (fwd("refuse-a-alpha"), set_a(alpha=0.5), "pair"),
        "a-m": (fwd("refuse-a-m"), set_a(M=100), "pair"),
        "a-resid": (fwd("refuse-a-resid"), resid_on_a, "pair"),
        "b-ldc": (fwd("refuse-b-ldc"), set_b(ldc=72), "pair"),
        "a-bits2-without-lrelu2": (fwd("refuse-a-bits2"), bits2_without_lrelu2, "pair"),
        "a-mask-and-maskbits": (bwd("refuse-a-masks"), mask_and_maskbits, "pair"),
        "b-act-slope": (fwd("refuse-b-slope"), set_b(act_slope=1.5), "pair"),
        "b-resid-inv-slope": (fwd("refuse-b-inv"), set_b(resid_inv_slope=0.5), "pair"),
        "a-ldxb-narrow": (bwd("refuse-a-ldxb"), set_a(ldxb=4), "pair"),
        "a-ldxb-unaligned": (bwd("refuse-a-ldxb9"), set_a(ldxb=9), "pair"),
        "b-ldxb-unaligned": (bwd("refuse-b-ldxb9"), set_b(ldxb=9), "pair"),
        "zero-rows-separate-r": (fwd("refuse-zero-rows", sep_r=True), zero_rows, "dead"),
    }


@pytest.mark.parametrize("what", list(_refusals()))
def test_refusals(what):
    """descriptors the fused pair does not take: a non-zero return, no kernel launched, every buffer as it was"""
    build, mutate, how = _refusals()[what]
    case = P.PairCase("refuse-" + what, "refuse", build, how)
    adt = _adt()
    problems, bufs, _ = case.data(adt)
    p = SimpleNamespace(a=SimpleNamespace(**vars(problems[0].a)), b=SimpleNamespace(**vars(problems[0].b)), dead=problems[0].dead)
    if mutate is not None:
        mutate(p)
    dev = _upload_case(case, bufs, adt)
    init = {k: v.cpu().clone() for k, v in dev.items()}
    rc, _ = _launch(case, [p], dev, how)
    torch.cuda.synchronize()
    assert rc != 0, what
    for k, v in dev.items():
        assert torch.equal(v.cpu(), init[k]), (what, k)
