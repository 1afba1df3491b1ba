"""-m gpu: the row kernels around the U-Net's attention, each through its C-ABI test hook against a float64 reference on the same
16-bit-rounded inputs: softmax (fp32 and 16-bit scores), the three transpose kernels (bit-exact), rowdot, LayerNorm and GEGLU.

Every output buffer is pre-filled with a sentinel bit pattern and checked outside the written region.  No tolerance is taken from a
kernel's output: each comes from the number formats (eps = unit roundoff of the activation type, `tiny` = its smallest subnormal) or,
for LayerNorm's E[x^2] - mean^2 variance, from a CPU emulation of that formula (test_layernorm_constant_comes_from_the_cpu_emulation,
which runs without a GPU)."""
import ctypes as C
import math

import pytest
import torch

gpu = pytest.mark.gpu
SENT16 = 0x7B7B                      # untouched 16-bit elements (finite in fp16 and bf16)
SENT32 = 0x7B7B7B7B                  # untouched fp32 elements


def _L():
    from diffmusic_amd import _lib as L
    return L


def _adt():
    return _L().act_dtype()


def _eps():
    return torch.finfo(_adt()).eps / 2


def _tiny():
    return torch.finfo(_adt()).smallest_normal * torch.finfo(_adt()).eps


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _out16(n):
    return torch.full((n,), SENT16, dtype=torch.int16, device="cuda")


def _pad8(n):
    return (n + 7) // 8 * 8


def _refused(rc, what, match):
    L = _L()
    assert rc != 0, what
    assert L.lib().dmx_last_error(), what
    with pytest.raises(L.DmxError, match=match):
        L.check(rc, what)


# ------------------------------------------------------------------------------------------------------------------ softmax
SOFTMAX_N = [4, 8, 252, 1000, 1020, 1024, 1028, 4096]       # one-wave-per-row kernel up to 1024, block-per-row kernel above
SOFTMAX_ROWS = [1, 3, 5, 1001]                              # live and dead rows inside one workgroup of four


def _softmax_bias(nb, N):
    """nb bias rows, each with its own run of -10000 (key 0 and key N - 1 stay live)."""
    b = torch.zeros(nb, N)
    for j in range(nb):
        lo = 1 + (j * 37) % max(1, N // 2)
        b[j, lo:min(N - 1, lo + max(1, N // 3))] = -10000.0
    return b


def _softmax_run(variant, S, bias, rows, N, rpb, in_place=False):
    """S: (rows, N) fp32 (CPU).  -> (P (rows, ldp) int16 bits on the CPU, guard (must be the sentinel), the scores as the kernel saw them)."""
    L = _L()
    ldp = _pad8(N)
    guard = 64
    bd = bias.cuda().contiguous() if bias is not None else None
    if variant == "fp32":
        lds = N + 4                                                          # a row stride that is not N
        Sd = torch.zeros(rows, lds)
        Sd[:, :N] = S
        Sd = Sd.cuda()
        out = _out16(rows * ldp + guard)
        rc = L.lib().dmx_softmax_raw(_p(Sd), _p(out), _p(bd), rows, N, lds, ldp, rpb, _st())
        seen = S.double()
    else:
        Sa = torch.full((rows, ldp), float("nan"), dtype=_adt())            # the padding columns of the score buffer are never read
        Sa[:, :N] = S.to(_adt())
        seen = Sa[:, :N].double()
        if in_place:
            out = _out16(rows * ldp + guard)
            out[:rows * ldp] = Sa.view(torch.int16).reshape(-1).cuda()
            rc = L.lib().dmx_softmax_act_raw(_p(out), _p(out), _p(bd), rows, N, ldp, rpb, _st())
        else:
            Sd = Sa.cuda()
            out = _out16(rows * ldp + guard)
            rc = L.lib().dmx_softmax_act_raw(_p(Sd), _p(out), _p(bd), rows, N, ldp, rpb, _st())
    torch.cuda.synchronize()
    L.check(rc, "softmax")
    o = out.cpu()
    return o[:rows * ldp].view(rows, ldp), o[rows * ldp:], seen


def _softmax_check(name, Pbits, guard, seen, bias, rows, N, rpb):
    assert (guard == SENT16).all(), name
    assert (Pbits[:, N:] == 0).all(), name                                   # the key padding [N, ldp) is exactly zero
    s = seen
    if bias is not None:
        s = s + bias.double()[torch.arange(rows) // rpb]
    p = torch.softmax(s, dim=-1)
    P = Pbits[:, :N].contiguous().view(_adt()).double()
    assert torch.isfinite(P).all(), name
    r = (P - p).abs() / (1.5 * _eps() * p + _tiny() / 2)
    ratio = r.max().item()
    normal = r[p >= torch.finfo(_adt()).smallest_normal].max().item()        # (a half-subnormal rounding alone reaches 1 - 1.5 eps)
    print(f"softmax {name}: max |P - p| / (1.5 eps p + tiny / 2) = {ratio:.3f} ({normal:.3f} over the normal range)")
    assert ratio <= 1.0, (name, ratio)


@gpu
@pytest.mark.parametrize("variant", ["fp32", "act"])
@pytest.mark.parametrize("N", SOFTMAX_N)
def test_softmax_rows(variant, N):
    g = torch.Generator().manual_seed(N)
    for rows in SOFTMAX_ROWS:
        S = 3.0 * torch.randn(rows, N, generator=g)
        Pbits, guard, seen = _softmax_run(variant, S, None, rows, N, 1)
        _softmax_check(f"{variant} N {N} rows {rows}", Pbits, guard, seen, None, rows, N, 1)


@gpu
@pytest.mark.parametrize("variant", ["fp32", "act"])
@pytest.mark.parametrize("N,rows,rpb", [(252, 41, 1), (252, 41, 7), (252, 40, 20), (1028, 15, 1), (1028, 15, 7), (1028, 16, 8)])
def test_softmax_bias_rows(variant, N, rows, rpb):
    """colbias with runs of -10000: row r uses bias row r / rows_per_bias (1; 7, not a divisor of the row count; heads * Nq)."""
    g = torch.Generator().manual_seed(N + rows + rpb)
    S = 3.0 * torch.randn(rows, N, generator=g)
    bias = _softmax_bias((rows + rpb - 1) // rpb, N)
    Pbits, guard, seen = _softmax_run(variant, S, bias, rows, N, rpb)
    _softmax_check(f"{variant} N {N} rows {rows} rows_per_bias {rpb}", Pbits, guard, seen, bias, rows, N, rpb)


@gpu
@pytest.mark.parametrize("N,rows", [(252, 5), (1000, 1001), (1028, 3), (4096, 5)])
def test_softmax_act_in_place_equals_out_of_place(N, rows):
    g = torch.Generator().manual_seed(N)
    S = 3.0 * torch.randn(rows, N, generator=g)
    bias = _softmax_bias((rows + 6) // 7, N)
    a, ga, _ = _softmax_run("act", S, bias, rows, N, 7)
    b, gb, _ = _softmax_run("act", S, bias, rows, N, 7, in_place=True)
    assert torch.equal(a, b) and (ga == SENT16).all() and (gb == SENT16).all()


@gpu
@pytest.mark.parametrize("N,ldp", [(6, 8), (4100, 4104), (8, 10)])
def test_softmax_refusals(N, ldp):
    L = _L()
    S32 = torch.zeros(4 * 4200, device="cuda")
    S16 = torch.zeros(4 * 4200, dtype=_adt(), device="cuda")
    out = _out16(4 * 4200)
    _refused(L.lib().dmx_softmax_raw(_p(S32), _p(out), None, 4, N, _pad8(N), ldp, 1, _st()), f"softmax N {N} ldp {ldp}", "softmax")
    _refused(L.lib().dmx_softmax_act_raw(_p(S16), _p(out), None, 4, N, ldp, 1, _st()), f"softmax_act N {N} ldp {ldp}", "softmax")
    torch.cuda.synchronize()
    assert (out == SENT16).all()


# ------------------------------------------------------------------------------------------------------------------ transpose
def _pattern(n):
    """Distinct 16-bit values per element (an odd multiplier is a bijection mod 2^16; runs longer than 65536 repeat far apart)."""
    return ((torch.arange(n, dtype=torch.int64) * 40503 + 12345) & 0xFFFF).to(torch.int32).to(torch.int16)


def _transpose_run(R, Cc, ldi, ldo, Z=1, Zi=1, sIo=None, sIi=0, sOo=None, sOi=0, in_off=0, in_elems=None, out_rows_alloc=None):
    """-> (input (CPU int16, flat), output (CPU int16, flat)).  Default batch strides: packed."""
    L = _L()
    sIo = R * ldi if sIo is None else sIo
    sOo = (out_rows_alloc or Cc) * ldo if sOo is None else sOo
    in_elems = in_elems or (Z // Zi) * sIo + Zi * sIi + 8
    out_elems = (Z // Zi) * sOo + Zi * sOi + 64
    x = _pattern(in_elems)
    xd = x.cuda()
    out = _out16(out_elems)
    rc = L.lib().dmx_transpose_raw(C.c_void_p(xd.data_ptr() + 2 * in_off), _p(out), R, Cc, ldi, ldo, Z, Zi, sIo, sIi, sOo, sOi, _st())
    torch.cuda.synchronize()
    L.check(rc, "transpose")
    return x, out.cpu()


def _transpose_expect(x, out_elems, R, Cc, ldi, ldo, Z, Zi, sIo, sIi, sOo, sOi, in_off, zero_pad):
    """The sentinel everywhere, out[z][c][r] = in[z][r][c], and (vector kernels) zeros in the columns [R, pad8(R)) of every written row."""
    want = torch.full((out_elems,), SENT16, dtype=torch.int16)
    for z in range(Z):
        zo, zi = divmod(z, Zi)
        src = torch.as_strided(x, (R, Cc), (ldi, 1), in_off + zo * sIo + zi * sIi)
        dst = torch.as_strided(want, (Cc, _pad8(R) if zero_pad else R), (ldo, 1), zo * sOo + zi * sOi)
        if zero_pad:
            dst[:, R:] = 0
        dst[:, :R] = src.t()
    return want


@gpu
@pytest.mark.parametrize("name,R,Cc,ldi,ldo,Z,zero_pad", [
    ("tile32: unaligned ldi / ldo, ragged in both directions, two matrices", 50, 33, 33, 51, 2, False),
    ("tile64: R = 77 into ldo = 80, columns 77 .. 79 written as zeros", 77, 64, 64, 80, 1, True),
    ("tile64: C = 61 of ldi = 64, the scalar tail of a partial 8-chunk", 64, 61, 64, 64, 1, True),
    ("tile128: ragged in both directions", 1030, 1027, 1032, 1032, 1, True)])
def test_transpose_is_bit_exact(name, R, Cc, ldi, ldo, Z, zero_pad):
    rows_alloc = _pad8(Cc)                           # output rows [C, pad8(C)) exist and must keep the sentinel
    sIo, sOo = R * ldi, rows_alloc * ldo
    x, out = _transpose_run(R, Cc, ldi, ldo, Z=Z, sIo=sIo, sOo=sOo)
    want = _transpose_expect(x, out.numel(), R, Cc, ldi, ldo, Z, 1, sIo, 0, sOo, 0, 0, zero_pad)
    assert torch.equal(out, want), name


@gpu
def test_transpose_batched_v_slice_as_the_attention_calls_it():
    """Z = B * heads, Zi = heads; the input is the V slice of a fused (B, Nk, 3C) buffer, the output (Z, dh, pad8(Nk))."""
    B, heads, dh, Nk = 2, 3, 24, 50
    Cc, ldv, Nkp = heads * dh, 3 * heads * dh, _pad8(Nk)
    args = dict(Z=B * heads, Zi=heads, sIo=Nk * ldv, sIi=dh, sOo=heads * dh * Nkp, sOi=dh * Nkp)
    x, out = _transpose_run(Nk, dh, ldv, Nkp, in_off=2 * Cc, in_elems=B * Nk * ldv, **args)
    want = _transpose_expect(x, out.numel(), Nk, dh, ldv, Nkp, args["Z"], heads, args["sIo"], dh, args["sOo"], args["sOi"], 2 * Cc, True)
    assert torch.equal(out, want)


# ------------------------------------------------------------------------------------------------------------------ rowdot
@gpu
@pytest.mark.parametrize("Cc", [8, 64, 512, 520])            # one lane; one pass; the full 512-column pass; a second, partial pass
def test_rowdot(Cc):
    L = _L()
    g = torch.Generator().manual_seed(Cc)
    lda, ldb = Cc + 8, Cc + 24
    for rows in (1, 5, 1003):
        a = torch.full((rows, lda), float("nan"), dtype=_adt())
        b = torch.full((rows, ldb), float("nan"), dtype=_adt())
        a[:, :Cc] = torch.randn(rows, Cc, generator=g).to(_adt())
        b[:, :Cc] = torch.randn(rows, Cc, generator=g).to(_adt())
        ad, bd = a.cuda(), b.cuda()
        out = torch.full((rows + 16,), SENT32, dtype=torch.int32, device="cuda")
        L.check(L.lib().dmx_rowdot_raw(_p(ad), _p(bd), _p(out), rows, Cc, lda, ldb, _st()), "rowdot")
        torch.cuda.synchronize()
        o = out.cpu()
        assert (o[rows:] == SENT32).all()
        prod = a[:, :Cc].double() * b[:, :Cc].double()
        err = (o[:rows].view(torch.float32).double() - prod.sum(-1)).abs()
        bound = (Cc + 8) * 2.0 ** -24 * prod.abs().sum(-1)               # the standard fp32 summation bound
        ratio = (err / bound).max().item()
        print(f"rowdot C {Cc} rows {rows}: max err / ((C + 8) 2^-24 sum |a b|) = {ratio:.4f}")
        assert ratio <= 1.0, (Cc, rows, ratio)


@gpu
@pytest.mark.parametrize("Cc,lda,ldb", [(12, 16, 16), (8, 12, 16), (8, 16, 20)])
def test_rowdot_refusals(Cc, lda, ldb):
    L = _L()
    a = torch.zeros(64, dtype=_adt(), device="cuda")
    out = torch.full((16,), SENT32, dtype=torch.int32, device="cuda")
    _refused(L.lib().dmx_rowdot_raw(_p(a), _p(a), _p(out), 2, Cc, lda, ldb, _st()), "rowdot", "rowdot")
    torch.cuda.synchronize()
    assert (out == SENT32).all()


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
LN_C = [8, 64, 504, 512, 520, 1280]          # one lane; partial wave; just below / at / just above one 512-column pass; three passes
LN_ROWS = [1, 5, 1003]
LN_EPS = 1e-5
# The kernel takes the variance as E[x^2] - mean^2 in fp32, whose cancellation error grows with E[x^2] / var.  The bound is
#     eps |ref| + |ref - beta| K 2^-24 E[x^2] / var
# with K = twice the largest factor (err - eps |ref|)+ / (|ref - beta| 2^-24 E[x^2] / var) of a CPU fp32 emulation of that formula
# (sums in the order of one wave: 8 consecutive columns per lane and pass, then the xor butterfly; the 16-bit store included) over
# these very rows and both activation types.  test_layernorm_constant_comes_from_the_cpu_emulation re-derives the figure (117.9, at
# fp16, C = 1280, 1003 rows) on every run.  The factor is this large because the fp32 error of the MEAN, an absolute
# ~2^-24 sqrt(E[x^2] / var) per element, is measured against |ref - beta|, which vanishes where x is close to the row mean.
LN_K = 236.0


def _ln_inputs(Cc, rows, adt):
    g = torch.Generator().manual_seed(100 * Cc + rows)
    x = (0.2 * torch.randn(rows, Cc, generator=g) + 3.0 * torch.randn(rows, 1, generator=g)).to(adt)     # rows with a common offset
    gamma = 1.0 + 0.1 * torch.randn(Cc, generator=g)
    beta = 0.1 * torch.randn(Cc, generator=g)
    return x, gamma, beta


def _ln_reference(x, gamma, beta):
    """-> (ref, E[x^2] / var) in float64."""
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    ref = (xd - mean) / torch.sqrt(var + LN_EPS) * gamma.double() + beta.double()
    return ref, (xd * xd).mean(-1, keepdim=True) / var


def _wave_sum_fp32(f):
    """Row sums (rows, 1) of fp32 f (rows, C) in the order of one 64-lane wave: lane l adds columns 512 p + 8 l .. + 7 pass by pass,
    then the lanes add through the xor butterfly 32, 16, .. 1."""
    rows, Cc = f.shape
    passes = (Cc + 511) // 512
    fp = torch.zeros(rows, passes * 512)
    fp[:, :Cc] = f
    fp = fp.view(rows, passes, 64, 8)
    acc = torch.zeros(rows, 64)
    for p in range(passes):
        for i in range(8):
            acc = acc + fp[:, p, :, i]
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, torch.arange(64) ^ o]
    return acc[:, :1]


def _ln_emulated_factor(Cc, rows, adt):
    x, gamma, beta = _ln_inputs(Cc, rows, adt)
    ref, ratio = _ln_reference(x, gamma, beta)
    xf = x.float()
    mean = _wave_sum_fp32(xf) / Cc
    var = (_wave_sum_fp32(xf * xf) / Cc - mean * mean).clamp_min(0.0)
    y = ((xf - mean) * torch.rsqrt(var + LN_EPS) * gamma + beta).to(adt).double()
    rem = ((y - ref).abs() - torch.finfo(adt).eps / 2 * ref.abs()).clamp_min(0.0)
    term = (ref - beta.double()).abs() * 2.0 ** -24 * ratio
    return torch.where(rem > 0, rem / term.clamp_min(1e-300), torch.zeros_like(rem)).max().item()


def test_layernorm_constant_comes_from_the_cpu_emulation():
    worst = max(_ln_emulated_factor(Cc, rows, adt) for Cc in LN_C for rows in LN_ROWS for adt in (torch.float16, torch.bfloat16))
    print(f"layernorm: largest emulated factor {worst:.3f}, K = {LN_K}")
    assert abs(LN_K - 2.0 * worst) <= 0.01 * LN_K, worst


@gpu
@pytest.mark.parametrize("Cc", LN_C)
def test_layernorm(Cc):
    L = _L()
    for rows in LN_ROWS:
        x, gamma, beta = _ln_inputs(Cc, rows, _adt())
        xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
        out = _out16(rows * Cc + 64)
        L.check(L.lib().dmx_layernorm_raw(_p(xd), _p(out), _p(gd), _p(bd), rows, Cc, LN_EPS, _st()), "layernorm")
        torch.cuda.synchronize()
        o = out.cpu()
        assert (o[rows * Cc:] == SENT16).all()
        y = o[:rows * Cc].view(_adt()).view(rows, Cc).double()
        ref, ratio = _ln_reference(x, gamma, beta)
        bound = _eps() * ref.abs() + (ref - beta.double()).abs() * LN_K * 2.0 ** -24 * ratio        # K = 236 (see LN_K)
        r = ((y - ref).abs() / bound).max().item()
        print(f"layernorm C {Cc} rows {rows}: max err / bound = {r:.3f} (largest E[x^2] / var {ratio.max().item():.0f})")
        assert torch.isfinite(y).all() and r <= 1.0, (Cc, rows, r)


@gpu
def test_layernorm_refusal():
    L = _L()
    x = torch.zeros(64, dtype=_adt(), device="cuda")
    w = torch.zeros(64, device="cuda")
    out = _out16(64)
    _refused(L.lib().dmx_layernorm_raw(_p(x), _p(out), _p(w), _p(w), 2, 12, LN_EPS, _st()), "layernorm C 12", "layernorm")
    torch.cuda.synchronize()
    assert (out == SENT16).all()


# ------------------------------------------------------------------------------------------------------------------ GEGLU
def _geglu_gates(n, adt, g):
    """Gates over [-10, 10] (erf saturated at both ends), +0 / -0, the subnormal range of the activation type, and N(0, 1)."""
    tiny = torch.finfo(adt).smallest_normal * torch.finfo(adt).eps
    special = torch.tensor([0.0, -0.0, 10.0, -10.0, tiny, -tiny, 3 * tiny, -5 * tiny, 0.5 * torch.finfo(adt).smallest_normal,
                            -0.75 * torch.finfo(adt).smallest_normal])
    gates = torch.cat([torch.linspace(-10.0, 10.0, n // 2), torch.randn(n - n // 2, generator=g)])
    gates = gates[torch.randperm(n, generator=g)]
    m = min(n, special.numel())
    gates[:m] = special[:m]
    return gates.to(adt)


@gpu
@pytest.mark.parametrize("I", [8, 1280, 2560])
def test_geglu(I):
    L = _L()
    g = torch.Generator().manual_seed(I)
    for rows in (1, 1003):
        val = torch.randn(rows, I, generator=g).to(_adt())
        gate = _geglu_gates(rows * I, _adt(), g).view(rows, I)
        if rows * I >= 16:
            val.view(-1)[:10] = 1.0                                      # the special gates meet a plain value
        x = torch.cat([val, gate], -1).contiguous()
        xd = x.cuda()
        out = _out16(rows * I + 64)
        L.check(L.lib().dmx_geglu_raw(_p(xd), _p(out), rows, I, _st()), "geglu")
        torch.cuda.synchronize()
        o = out.cpu()
        assert (o[rows * I:] == SENT16).all()
        y = o[:rows * I].view(_adt()).view(rows, I).double()
        gd = gate.double()
        ref = val.double() * 0.5 * gd * torch.special.erfc(-gd / math.sqrt(2.0))       # = g/2 (1 + erf(g / sqrt 2)), free of cancellation
        ratio = (y - ref).abs() / (1.5 * _eps() * ref.abs() + _tiny() / 2)
        worst = ratio.argmax()
        normal = ratio[ref.abs() >= torch.finfo(_adt()).smallest_normal].max().item() if rows * I > 8 else float("nan")
        print(f"geglu I {I} rows {rows}: max err / (1.5 eps |ref| + tiny / 2) = {ratio.max().item():.3f} at gate {gd.view(-1)[worst].item():.4g}"
              f" ({normal:.3f} over the normal range)")
        assert torch.isfinite(y).all() and ratio.max().item() <= 1.0, (I, rows, ratio.max().item())


@gpu
def test_geglu_refusal():
    L = _L()
    x = torch.zeros(64, dtype=_adt(), device="cuda")
    out = _out16(64)
    _refused(L.lib().dmx_geglu_raw(_p(x), _p(out), 2, 12, _st()), "geglu I 12", "geglu")
    torch.cuda.synchronize()
    assert (out == SENT16).all()
