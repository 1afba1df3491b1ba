"""Shared by tests/test_attention_bound_host.py (CPU) and tests/test_gpu_attention_edges.py / tests/test_gpu_attention.py (GPU):
the case table of the fused attention kernel's edge tests, their inputs, the float64 reference and its element-wise error bound.

Bound (derived from the number formats, never from the kernel's output).  With eps the unit roundoff of the 16-bit activation type,
p_ij the exact softmax probabilities and l_i = sum_j exp(s_ij - max_j s_ij):
    u[i, d]   = eps * sum_j p_ij |v_jd|
    sub[i, d] = Nk * (smallest subnormal) / 2 * max_j |v_jd| / l_i
    |o - ref| <= 3 u + sub
The kernel rounds every un-normalised probability once to the activation type (relative eps; an absolute half subnormal below the
normal range) and every output once (eps |o| <= u); sums and rescales are fp32.  That is 2 u + sub; the third u is the margin for the
fp32 sums and exp2."""
import math
import zlib
from collections import namedtuple

import torch

KB = 64                                   # keys per block of the kernel's online softmax
CLASS_TOPS = (32, 48, 64, 80, 96)         # largest head dim of each template class of the kernel

# layout: how q / k / v lie in memory --
#   "plain": three packed (B, N, C) tensors;
#   "qkv":   slices of one fused (B, N, 3C) buffer at channel offsets 0, C, 2C (Nq == Nk), ldq = ldk = ldv = 3C;
#   "ctx":   q packed, k and v slices of one (B, Nk, 2C + 8) buffer at offsets 0 and C (8 spare columns), ldk = ldv = 2C + 8.
# inp: "randn"; "peaked" (q scaled by 6); "ends" (peaked, and each row's largest logit forced into the last key block for even
#      rows and into block 0 for odd rows: the rescale by alpha runs in both directions).
# mask: None or (lo, hi): keys lo .. hi - (b % 2) of batch b carry the bias -10000 (the engine's (1 - mask) * -10000), all others 0.
# qt: the query-tile form the launch rule must take (1: 64 queries per workgroup; 2: 128).
# Every case with Nk >= 512 has the hot key v[Nk - 1] = 4 in every channel.
Case = namedtuple("Case", "name B heads dh Nq Nk ldq ldk ldv inp mask qt layout")


def _case(name, B, heads, dh, Nq, Nk, layout="plain", inp="randn", mask=None):
    C = heads * dh
    ldq, ldk, ldv = {"plain": (C, C, C), "qkv": (3 * C, 3 * C, 3 * C), "ctx": (C, 2 * C + 8, 2 * C + 8)}[layout]
    assert layout != "qkv" or Nq == Nk
    qt = 1 if (-(-Nq // 128) * B * heads <= 256 or Nq <= 64) else 2       # the documented grid rule (flash_attn.hip launch_fa)
    return Case(name, B, heads, dh, Nq, Nk, ldq, ldk, ldv, inp, mask, qt, layout)


CASES = [
    # head dims below the top of their template class, two or more heads (the d < dh guards and the zero fill of d >= dh do real work)
    _case("dh8", 1, 3, 8, 130, 77),
    _case("dh16-qkv", 2, 2, 16, 65, 65, "qkv"),
    _case("dh24-ctx", 1, 2, 24, 130, 77, "ctx"),
    _case("dh40-peaked", 1, 3, 40, 64, 129, inp="peaked"),
    _case("dh56-qkv", 2, 2, 56, 127, 127, "qkv"),
    _case("dh72-ctx-ends-mask", 2, 2, 72, 129, 200, "ctx", "ends", (8, 198)),
    _case("dh88-qkv", 1, 2, 88, 130, 130, "qkv"),
    # query edges (Nq = 64, 127, 129, 130 are above)
    _case("nq1", 2, 2, 32, 1, 63),
    _case("nq63", 1, 2, 32, 63, 8),
    _case("nq65-nk1", 1, 2, 48, 65, 1),
    _case("nq128", 1, 2, 16, 128, 128, "qkv"),
    # the launch rule: 2 x 129 workgroups of 128 queries > 256 -> QT = 2, whose second workgroup holds 2 live queries and three dead
    # waves; the same Nq on a small grid takes QT = 1
    _case("qt2-dh8", 43, 3, 8, 130, 65),
    _case("qt2-dh40-ctx", 65, 2, 40, 130, 50, "ctx", "randn", (3, 40)),
    _case("qt1-nq130", 2, 2, 32, 130, 64, inp="peaked"),
    # key edges (Nk = 1, 8, 63, 64, 65, 128, 129, 200 are above)
    _case("nk50", 1, 2, 64, 70, 50, "ctx"),
    # the product's masks: [SOS live | tokens | padding masked | EOS live].  Nk = 200 with keys 8 .. 198 masked is above (blocks 1 and 2
    # dead, block 3's only live key its last valid one); here keys 1 .. 127: two dead blocks' worth and a live ragged tail
    _case("nk130-mask", 1, 2, 32, 33, 130, "plain", "randn", (1, 127)),
    _case("nk200-ends", 1, 2, 32, 66, 200, "plain", "ends"),
    # a dead block 0: keys 0 .. 63 masked, key 64 onward live
    _case("block0-dead", 2, 2, 24, 70, 100, "ctx", "randn", (0, 63)),
    # long key runs with the hot key in the ragged last block
    _case("nk1000-hot", 1, 2, 32, 130, 1000),
    _case("nk520-hot-peaked-ctx", 1, 2, 24, 64, 520, "ctx", "peaked"),
]
BY_NAME = {c.name: c for c in CASES}


def act_eps(adt):
    return torch.finfo(adt).eps / 2


def act_tiny(adt):
    """Smallest positive subnormal of the activation type."""
    return torch.finfo(adt).smallest_normal * torch.finfo(adt).eps


def make_bias(case):
    if case.mask is None:
        return None
    lo, hi = case.mask
    bias = torch.zeros(case.B, case.Nk, dtype=torch.float32)
    for b in range(case.B):
        bias[b, lo:hi - (b % 2) + 1] = -10000.0
    return bias


def _heads(x, heads):
    B, N, C = x.shape
    return x.view(B, N, heads, C // heads).transpose(1, 2)           # (B, heads, N, dh)


def make_inputs(case, adt):
    """q (B, Nq, C), k, v (B, Nk, C) rounded to `adt` (logical, packed), bias (B, Nk) fp32 or None."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    B, heads, dh, Nq, Nk = case.B, case.heads, case.dh, case.Nq, case.Nk
    C = heads * dh
    q = torch.randn(B, Nq, C, generator=g)
    k = torch.randn(B, Nk, C, generator=g)
    v = torch.randn(B, Nk, C, generator=g)
    bias = make_bias(case)
    if case.inp in ("peaked", "ends"):
        q = q * 6.0
    if Nk >= 512:
        v[:, Nk - 1, :] = 4.0
    if case.inp == "ends":
        assert Nk > KB
        # channel 0 of every head steers: it is zero in every key but key 0 (-1) and key Nk - 1 (+1), so q[i, 0] = +g lifts the
        # logit of the last key and -g that of key 0 without touching any other logit
        qh, kh = _heads(q, heads), _heads(k, heads)
        kh[..., 0] = 0.0
        kh[:, :, 0, 0] = -1.0
        kh[:, :, Nk - 1, 0] = 1.0
        qh[..., 0] = 0.0
        scale = 1.0 / math.sqrt(dh)
        qr, kr = qh.to(adt).double(), kh.to(adt).double()
        s = qr @ kr.transpose(-1, -2) * scale
        if bias is not None:
            s = s + bias.double()[:, None, None, :]
        rows = torch.arange(Nq)
        even = (rows % 2 == 0)[None, None, :]
        tgt = torch.where(even, s[..., Nk - 1], s[..., 0])
        others = s.clone()
        others[..., 0] = torch.where(even, others[..., 0], -float("inf"))          # the other end only loses by the gain: it competes
        others[..., Nk - 1] = torch.where(even, -float("inf"), others[..., Nk - 1])
        gain = ((others.amax(-1) + 3.0 - tgt) / scale).clamp_min(0.0)
        qh[..., 0] = torch.where(even, gain, -gain).float()
    q, k, v = q.to(adt), k.to(adt), v.to(adt)
    if case.inp == "ends":
        s = logits(q, k, bias, heads)
        blk = s.argmax(-1) // KB
        want = torch.where(torch.arange(Nq) % 2 == 0, (Nk - 1) // KB, 0)
        assert torch.equal(blk, want.expand_as(blk)), "the steering channel did not place the row maxima"
    return q, k, v, bias


def logits(q, k, bias, heads):
    """float64 logits (B, heads, Nq, Nk) of 16-bit q, k with the bias added as given."""
    qh, kh = _heads(q.double(), heads), _heads(k.double(), heads)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(qh.shape[-1])
    if bias is not None:
        s = s + bias.double()[:, None, None, :]
    return s


def _merge(o):
    B, H, N, dh = o.shape
    return o.transpose(1, 2).reshape(B, N, H * dh)


def attend(s, v, heads):
    """Exact float64 softmax(s) v -> (B, Nq, C), from logits (B, heads, Nq, Nk) and 16-bit v (B, Nk, C)."""
    vh = _heads(v.double(), heads)
    pt = torch.exp(s - s.amax(-1, keepdim=True))
    return _merge((pt / pt.sum(-1, keepdim=True)) @ vh)


def reference(q, k, v, bias, heads, adt):
    """(ref, bound): float64 softmax attention on the given 16-bit q, k, v and the element-wise bound 3u + sub, both (B, Nq, C)."""
    s = logits(q, k, bias, heads)
    vh = _heads(v.double(), heads)
    Nk = vh.shape[2]
    pt = torch.exp(s - s.amax(-1, keepdim=True))
    l = pt.sum(-1, keepdim=True)
    p = pt / l
    ref = p @ vh
    u = act_eps(adt) * (p @ vh.abs())
    sub = Nk * act_tiny(adt) / 2 * vh.abs().amax(-2, keepdim=True) / l
    return _merge(ref), _merge(3 * u + sub)


def emulate(q, k, v, bias, heads, adt):
    """float64 model of the kernel's two roundings: keys in blocks of 64 under the running maximum, the un-normalised
    probabilities as fp32 values cast to the activation type, exact sums and rescales, and the output cast."""
    s = logits(q, k, bias, heads)
    vh = _heads(v.double(), heads)
    B, H, Nq, Nk = s.shape
    o = torch.zeros(B, H, Nq, vh.shape[-1], dtype=torch.float64)
    m = torch.full((B, H, Nq, 1), -float("inf"), dtype=torch.float64)
    l = torch.zeros(B, H, Nq, 1, dtype=torch.float64)
    for k0 in range(0, Nk, KB):
        sb = s[..., k0:k0 + KB]
        mn = torch.maximum(m, sb.amax(-1, keepdim=True))
        alpha = torch.exp(m - mn)
        pb = torch.exp(sb - mn).float()
        l = l * alpha + pb.double().sum(-1, keepdim=True)
        o = o * alpha + pb.to(adt).double() @ vh[:, :, k0:k0 + KB]
        m = mn
    return _merge((o / l).float().to(adt).double())


def class_top(dh):
    return next(t for t in CLASS_TOPS if dh <= t)


# ---- mutants of the reference: what a subtly wrong kernel would compute.  Each returns None where the case does not exercise the
# feature it breaks.
def mutant_drop_last_key(case, q, k, v, bias):
    if case.Nk < 2:
        return None
    s = logits(q, k, bias, case.heads)
    s[..., -1] = -float("inf")
    return attend(s, v, case.heads)


def mutant_ignore_one_bias(case, q, k, v, bias):
    if bias is None:
        return None
    lo, hi = case.mask
    b2 = bias.clone()
    assert (bias[:, (lo + hi) // 2] < 0).all()           # a key that is masked in every batch
    b2[:, (lo + hi) // 2] = 0.0
    return attend(logits(q, k, b2, case.heads), v, case.heads)


def mutant_next_head_channels(case, q, k, v, bias):
    """Missing d < dh guards: head h's q.k runs over class_top(dh) channels starting at h * dh, i.e. into the next head's
    (zeros past the last head's end)."""
    top = class_top(case.dh)
    if case.dh == top:
        return None
    pad = top - case.dh
    qd = torch.nn.functional.pad(q.double(), (0, pad))
    kd = torch.nn.functional.pad(k.double(), (0, pad))
    idx = (torch.arange(case.heads)[:, None] * case.dh + torch.arange(top)[None, :]).reshape(-1)
    qw, kw = qd[..., idx], kd[..., idx]                  # (B, N, heads * top): head h = its own dh channels + the next pad channels
    s = _heads(qw, case.heads) @ _heads(kw, case.heads).transpose(-1, -2) / math.sqrt(case.dh)
    if bias is not None:
        s = s + bias.double()[:, None, None, :]
    return attend(s, v, case.heads)


def mutant_key_row_off_by_one(case, q, k, v, bias):
    """A wrong key stride / batch offset: key j is read from row j + 1 (the values stay in place)."""
    if case.layout == "plain" or case.Nk < 2:
        return None
    return attend(logits(q, torch.roll(k, -1, dims=1), bias, case.heads), v, case.heads)


MUTANTS = {"drop_last_key": mutant_drop_last_key, "ignore_one_bias": mutant_ignore_one_bias,
           "next_head_channels": mutant_next_head_channels, "key_row_off_by_one": mutant_key_row_off_by_one}
