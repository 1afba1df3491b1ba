"""-m gpu: the fused forward attention kernel (C-ABI hook dmx_flash_attn_ld_raw) the way the U-Net calls it -- strided q / k / v, head
dims below the top of their template class, both query-tile forms, ragged query and key tails, the product's key masks -- against
float64 softmax attention on the CPU, element by element.

The case table, the reference and the bound |o - ref| <= 3u + sub live in tests/attention_cases.py; tests/test_attention_bound_host.py
validates that bound from the reference alone (an emulation of the kernel's roundings stays inside half of it; four mutants of the
reference leave it), so no tolerance here is taken from the kernel's output.

A key bias of -inf is outside the kernel's contract: the engine builds (1 - mask) * -10000 and nothing else, so -inf is not tested.
Neither is a row whose keys are all masked (the fp32 reference semantics are degenerate there as well)."""
import ctypes as C
import math

import pytest
import torch

from tests import attention_cases as AC

pytestmark = pytest.mark.gpu

SENTINEL = 0x7B7B               # bit pattern of untouched 16-bit output elements (finite in fp16 and bf16)
_ref_cache = {}


def _adt():
    from diffmusic_amd import _lib as L
    return L.act_dtype()


def _data(case):
    if case.name not in _ref_cache:
        q, k, v, bias = AC.make_inputs(case, _adt())
        ref, bound = AC.reference(q, k, v, bias, case.heads, _adt())
        _ref_cache[case.name] = (q, k, v, bias, ref, bound)
    return _ref_cache[case.name]


def _bits(t):
    return t.view(torch.int16)


def _pack(case, q, k, v, spare=0.0, extra_rows=0, layout=None):
    """Device buffers of the case's memory layout -> (keepalive, q_ptr, k_ptr, v_ptr, ldq, ldk, ldv).  `spare` fills the 8 spare
    columns of the context buffer; `extra_rows` NaN rows follow the Nk keys of K and V (B = 1 only)."""
    layout = layout or case.layout
    B, Nk, Cc = k.shape
    assert extra_rows == 0 or (B == 1 and layout != "qkv")
    nan_rows = torch.full((B, extra_rows, Cc), float("nan"), dtype=q.dtype)
    k, v = torch.cat([k, nan_rows], 1), torch.cat([v, nan_rows], 1)
    if layout == "plain":
        qd, kd, vd = q.cuda().contiguous(), k.cuda().contiguous(), v.cuda().contiguous()
        return (qd, kd, vd), qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), Cc, Cc, Cc
    if layout == "qkv":
        buf = torch.cat([q, k, v], -1).cuda().contiguous()
        return (buf,), buf.data_ptr(), buf.data_ptr() + 2 * Cc, buf.data_ptr() + 4 * Cc, 3 * Cc, 3 * Cc, 3 * Cc
    qd = q.cuda().contiguous()
    buf = torch.cat([k, v, torch.full((B, k.shape[1], 8), spare, dtype=q.dtype)], -1).cuda().contiguous()
    return (qd, buf), qd.data_ptr(), buf.data_ptr(), buf.data_ptr() + 2 * Cc, Cc, 2 * Cc + 8, 2 * Cc + 8


def _launch(qp, kp, vp, o, bias_d, B, Nq, Nk, ldq, ldk, ldv, Cc, heads, scale):
    from diffmusic_amd import _lib as L
    qt = C.c_int(-1)
    rc = L.lib().dmx_flash_attn_ld_raw(C.c_void_p(qp), C.c_void_p(kp), C.c_void_p(vp), C.c_void_p(o.data_ptr()),
                                       C.c_void_p(bias_d.data_ptr()) if bias_d is not None else None, B, Nq, Nk, ldq, ldk, ldv, Cc, heads,
                                       scale, C.byref(qt), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, qt.value


def _run(case, q, k, v, bias, guard=2, **pack):
    """-> (o (B, Nq, C) on the CPU, qt, guard rows before / after the output (must still hold the sentinel))."""
    from diffmusic_amd import _lib as L
    B, Nq, Cc = q.shape
    keep, qp, kp, vp, ldq, ldk, ldv = _pack(case, q, k, v, **pack)
    obuf = torch.full((B * Nq + 2 * guard, Cc), SENTINEL, dtype=torch.int16, device="cuda")
    o = obuf[guard:guard + B * Nq]
    bias_d = bias.cuda().contiguous() if bias is not None else None
    rc, qt = _launch(qp, kp, vp, o, bias_d, B, Nq, case.Nk, ldq, ldk, ldv, Cc, case.heads, 1.0 / math.sqrt(case.dh))
    L.check(rc, "flash_attn_ld")
    out = obuf.cpu()
    return out[guard:guard + B * Nq].view(_adt()).view(B, Nq, Cc), qt, torch.cat([out[:guard], out[guard + B * Nq:]])


def _check(name, o, ref, bound):
    assert torch.isfinite(o).all(), name
    ratio = ((o.double() - ref).abs() / bound).max().item()
    print(f"{name}: max |o - ref| / (3u + sub) = {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


IDS = [c.name for c in AC.CASES]


@pytest.mark.parametrize("case", AC.CASES, ids=IDS)
def test_every_element_is_within_the_bound(case):
    assert (case.ldq, case.ldk, case.ldv) == {"plain": (case.heads * case.dh,) * 3, "qkv": (3 * case.heads * case.dh,) * 3,
                                              "ctx": (case.heads * case.dh,) + (2 * case.heads * case.dh + 8,) * 2}[case.layout]
    q, k, v, bias, ref, bound = _data(case)
    o, qt, guard = _run(case, q, k, v, bias)
    print(f"{case.name}: qt_out = {qt}")
    assert qt == case.qt, (qt, case.qt)       # the launch rule still takes the form this case exists for
    assert (guard == SENTINEL).all()
    _check(case.name, o, ref, bound)


@pytest.mark.parametrize("case", [c for c in AC.CASES if c.dh < AC.class_top(c.dh)], ids=lambda c: c.name)
def test_nan_in_the_other_heads_changes_no_bit(case):
    """A missing d < dh guard mixes the next head's channels in: with every other head's q / k / v channels NaN, a head's output
    keeps its bits."""
    assert case.heads >= 2
    q, k, v, bias, ref, bound = _data(case)
    o, qt, _ = _run(case, q, k, v, bias)
    dh = case.dh
    for h in range(case.heads):
        qn, kn, vn = (torch.full_like(t, float("nan")) for t in (q, k, v))
        for src, dst in ((q, qn), (k, kn), (v, vn)):
            dst[..., h * dh:(h + 1) * dh] = src[..., h * dh:(h + 1) * dh]
        on, qtn, _ = _run(case, qn, kn, vn, bias)
        assert qtn == qt
        assert torch.equal(_bits(on[..., h * dh:(h + 1) * dh]), _bits(o[..., h * dh:(h + 1) * dh])), (case.name, h)


@pytest.mark.parametrize("case", [c for c in AC.CASES if c.layout == "ctx"], ids=lambda c: c.name)
def test_nan_in_the_spare_columns_changes_no_bit(case):
    q, k, v, bias, ref, bound = _data(case)
    o, qt, _ = _run(case, q, k, v, bias)
    on, qtn, _ = _run(case, q, k, v, bias, spare=float("nan"))
    assert qtn == qt and torch.equal(_bits(on), _bits(o))


@pytest.mark.parametrize("case", [c for c in AC.CASES if c.B == 1 and c.layout != "qkv"], ids=lambda c: c.name)
def test_rows_past_nk_are_never_used_and_rows_past_nq_never_written(case):
    """64 NaN rows behind K and V: "keys past Nk are zeros" must hold for V (where 0 * NaN would surface), and the rows around the
    output keep their sentinel."""
    q, k, v, bias, ref, bound = _data(case)
    o, qt, _ = _run(case, q, k, v, bias)
    on, qtn, guard = _run(case, q, k, v, bias, guard=8, extra_rows=64)
    assert torch.isfinite(on).all()
    assert qtn == qt and torch.equal(_bits(on), _bits(o))
    assert (guard == SENTINEL).all()


@pytest.mark.parametrize("case", [c for c in AC.CASES if c.layout != "plain"], ids=lambda c: c.name)
def test_strided_call_gives_the_bits_of_the_packed_call(case):
    q, k, v, bias, ref, bound = _data(case)
    o, qt, _ = _run(case, q, k, v, bias)
    op, qtp, _ = _run(case, q, k, v, bias, layout="plain")
    assert qtp == qt and torch.equal(_bits(op), _bits(o))


@pytest.mark.parametrize("case", [c for c in AC.CASES if c.B >= 2], ids=lambda c: c.name)
def test_a_clip_alone_matches_its_rows_in_the_batch(case):
    """Same query-tile form: the same bits.  Another form (the batch took QT = 2, the single clip QT = 1): within the bound."""
    q, k, v, bias, ref, bound = _data(case)
    o, qt, _ = _run(case, q, k, v, bias)
    b = case.B - 1
    o1, qt1, _ = _run(case, q[b:b + 1], k[b:b + 1], v[b:b + 1], bias[b:b + 1] if bias is not None else None)
    print(f"{case.name}: qt_out batch {qt}, clip alone {qt1}")
    assert qt1 == 1                          # one clip of these sizes never fills the chip
    if qt1 == qt:
        assert torch.equal(_bits(o1[0]), _bits(o[b]))
    else:
        _check(case.name + " (clip alone)", o1, ref[b:b + 1], bound[b:b + 1])


@pytest.mark.parametrize("what,kw", [("ldq", dict(ldq=68)), ("ldk", dict(ldk=132)), ("ldv", dict(ldv=140)), ("dh12", dict(Cc=24)),
                                     ("dh104", dict(Cc=208)), ("nk0", dict(Nk=0))])
def test_refusals_name_the_reason_and_launch_nothing(what, kw):
    from diffmusic_amd import _lib as L
    p = dict(B=1, Nq=16, Nk=16, ldq=256, ldk=256, ldv=256, Cc=64, heads=2)
    p.update(kw)
    buf = torch.zeros(3, 16 * 256, dtype=_adt(), device="cuda")
    o = torch.full((16, 256), SENTINEL, dtype=torch.int16, device="cuda")
    rc, qt = _launch(buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), o, None, p["B"], p["Nq"], p["Nk"], p["ldq"], p["ldk"], p["ldv"],
                     p["Cc"], p["heads"], 0.125)
    assert rc != 0 and qt == 0, (what, rc, qt)
    assert L.lib().dmx_last_error(), what
    with pytest.raises(L.DmxError, match="flash attention"):
        L.check(rc, what)
    assert (o == SENTINEL).all(), what
