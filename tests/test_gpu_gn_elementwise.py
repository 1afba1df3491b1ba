"""-m gpu: GroupNorm (+SiLU) forward and backward (csrc/elementwise.hip) and the two GEMM epilogues that feed them (EPI_GNSTATS / EPI_GNBWD,
csrc/gemm_epilogue.h) through the C-ABI test hooks, ELEMENT BY ELEMENT against the float64 model of tests/gn_cases.py on the same 16-bit
tensors.  Every output buffer is pre-filled with a sentinel (0x7B7B for 16-bit, NaN for stats / scale / shift / k0 / k1 and the partial-sum
buffers) and carries a guard beyond its declared size -- beyond dmx_groupnorm_scratch_floats and dmx_groupnorm_part_floats too; a case
passes when
  - stats, scale, shift, k0, k1 are written everywhere and within their bounds, the guards still hold their sentinels;
  - y is within its bound of the float64 model AND within one rounding (+ the fp32 slack of the affine) of act(x scale_k + shift_k) taken
    in float64 from the tape the kernel itself wrote -- what the backward recomputes;
  - dx is within its bound of the closed-form float64 backward, classic and producer routes; the tape is the float64 model's rounded to
    fp32 (so the backward is checked without the forward kernels), for ROUND_TRIP additionally the tape the forward kernel wrote;
  - every (image, slot, quad) partial sum of a producer launch is within its bound of the float64 sums of the stored tensor, an image's
    last, shorter slot included, and every other element of the buffer still holds NaN;
  - refused shapes leave every output untouched.
The bounds come from the number formats and the shapes (gn_cases docstring; tests/test_gn_bound_host.py validates them without a GPU);
every test prints its observed max err / bound per output.  The measured ratios are recorded in DESIGN.md section 5."""
import ctypes as C
import functools

import pytest
import torch

from tests import gn_cases as N
from tests.test_gpu_gn_combine import _forward_and_dgrad, _produce

pytestmark = pytest.mark.gpu
GUARD = 4096
BY_NAME = {c.name: c for c in N.CASES}


def _L():
    from diffmusic_amd import _lib as L
    return L


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sent16(n):
    return torch.full((n + GUARD,), N.SENT16, dtype=torch.int16, device="cuda")


def _nan(n):
    return torch.full((n + GUARD,), float("nan"), device="cuda")


def _out16(buf, shape, adt, what):
    """the declared part of a sentinel-filled 16-bit buffer as float64 on the CPU; asserts the guard"""
    n = 1
    for s in shape:
        n *= s
    h = buf.cpu()
    assert bool((h[n:] == N.SENT16).all()), f"{what}: written beyond its {n} elements"
    return h[:n].view(adt).double().view(*shape)


def _out32(buf, shape, what, written=True):
    n = 1
    for s in shape:
        n *= s
    h = buf.cpu()
    assert bool(torch.isnan(h[n:]).all()), f"{what}: written beyond its {n} elements"
    if written:
        assert bool(torch.isfinite(h[:n]).all()), f"{what}: {int((~torch.isfinite(h[:n])).sum())} of {n} elements not written (or not finite)"
    return h[:n].double().view(*shape)


def _check(what, got, ref, bound):
    err = (got - ref).abs()
    ok = err <= bound
    ratio = (err / bound.clamp_min(1e-300))
    worst = ratio.max().item() if ratio.numel() else 0.0
    if not bool(ok.all()):
        i = int(ratio.argmax())
        at = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements outside the bound, worst err / bound {worst:.3f} at {at}: "
                             f"got {got.flatten()[i].item():.9g} ref {ref.flatten()[i].item():.9g} bound {bound.flatten()[i].item():.3g}")
    return worst


def _report(tag, w):
    print(f"{tag}: max err / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in w.items()))


@functools.lru_cache(maxsize=2)
def _reference(name):
    """data, float64 forward model and its bound of a case, shared by its forward and backward tests"""
    c, adt = BY_NAME[name], _L().act_dtype()
    d = c.data(adt)
    r = N.forward(d.x, d.gamma, d.beta, c.G, c.eps, c.silu, with_y=c.with_y)
    b = N.forward_bound(d.x, d.gamma, d.beta, c.G, c.eps, c.silu, r, c.d, c.two_pass, adt, with_y=c.with_y)
    return d, r, b


def _run_forward(x, gamma, beta, B, P, Cc, G, eps, silu, with_y, parts=None):
    """dmx_groupnorm_raw, or dmx_groupnorm_parts_raw when parts = [(part, tm, P_region, nq, qoff, cq)] -> (y or None, mean, rstd, scale, shift)"""
    L, adt = _L(), _L().act_dtype()
    ybuf = _sent16(B * P * Cc) if with_y else None
    stats, scale, shift = _nan(B * G * 2), _nan(B * Cc), _nan(B * Cc)
    if parts is None:
        nscr = L.lib().dmx_groupnorm_scratch_floats(B, Cc, G)
        partial = _nan(nscr)
        L.check(L.lib().dmx_groupnorm_raw(_p(x), _p(ybuf), _p(gamma), _p(beta), _p(stats), _p(scale), _p(shift), _p(partial), B, P, Cc, G, eps,
                                          silu, _stream()), "groupnorm")
    else:
        geom, ptrs = [], []
        for part, tm, Pr, nq, qoff, cq in parts:
            geom += [tm, Pr, nq, qoff, cq, 0]
            ptrs.append(part.data_ptr())
        n = len(parts)
        L.check(L.lib().dmx_groupnorm_parts_raw(_p(x), _p(ybuf), _p(gamma), _p(beta), _p(stats), _p(scale), _p(shift), B, P, Cc, G, eps, silu, n,
                                                (C.c_void_p * n)(*ptrs), (C.c_int * (6 * n))(*geom), _stream()), "groupnorm_parts")
    torch.cuda.synchronize()
    if parts is None:
        _out32(partial, (nscr,), "scratch", written=False)
    st = _out32(stats, (B, G, 2), "stats")
    y = _out16(ybuf, (B, P, Cc), adt, "y") if with_y else None
    return y, st[..., 0], st[..., 1], _out32(scale, (B, Cc), "scale"), _out32(shift, (B, Cc), "shift")


def _run_backward(x, dy, add, mean, rstd, scale, shift, B, P, Cc, G, silu, parts=None):
    """dmx_groupnorm_bwd_raw from a tape given as float64 values of fp32 -> (dx, k0, k1)"""
    L, adt = _L(), _L().act_dtype()
    stats = torch.stack([mean, rstd], dim=2).float().cuda()
    sc, sf = scale.float().cuda(), shift.float().cuda()
    dxbuf, k0, k1 = _sent16(B * P * Cc), _nan(B * Cc), _nan(B * Cc)
    nscr = L.lib().dmx_groupnorm_scratch_floats(B, Cc, G)
    partial = _nan(nscr)
    if parts is None:
        n, ptrs, geom = 0, None, None
    else:
        n = len(parts)
        ptrs = (C.c_void_p * n)(*[p[0].data_ptr() for p in parts])
        geom = (C.c_int * (6 * n))(*[v for p in parts for v in (p[1], p[2], p[3], p[4], p[5], 0)])
    L.check(L.lib().dmx_groupnorm_bwd_raw(_p(x), _p(dy), _p(add), _p(dxbuf), _p(stats), _p(sc), _p(sf), _p(k0), _p(k1), _p(partial), B, P, Cc, G,
                                          silu, n, ptrs, geom, _stream()), "groupnorm_bwd")
    torch.cuda.synchronize()
    _out32(partial, (nscr,), "scratch", written=False)
    return _out16(dxbuf, (B, P, Cc), adt, "dx"), _out32(k0, (B, Cc), "k0"), _out32(k1, (B, Cc), "k1")


def _dev16(t):
    return t.to(_L().act_dtype()).cuda()


def _check_forward(tag, x, gamma, beta, G, silu, got, r, b, with_y):
    """stats / scale / shift / y against the model, and y against the kernel's own tape"""
    adt = _L().act_dtype()
    y, mean, rstd, scale, shift = got
    w = {"mean": _check(tag + " mean", mean, r.mean, b.mean), "rstd": _check(tag + " rstd", rstd, r.rstd, b.rstd),
         "scale": _check(tag + " scale", scale, r.scale, b.scale), "shift": _check(tag + " shift", shift, r.shift, b.shift)}
    if with_y:
        w["y"] = _check(tag + " y", y, r.y, b.y)
        gid = torch.arange(x.shape[2]) // (x.shape[2] // G)
        z = x * scale[:, None] + shift[:, None]
        yk = z * torch.sigmoid(z) if silu else z
        msb = (mean[:, gid] * scale).abs() + beta.abs()
        w["y|tape"] = _check(tag + " y against its own tape", y, yk, N.tape_bound(x, yk, scale, shift, msb, silu, adt))
    return w


@pytest.mark.parametrize("case", N.CASES, ids=repr)
def test_forward(case):
    c = case
    d, r, b = _reference(c.name)
    got = _run_forward(_dev16(d.x), d.gamma.float().cuda(), d.beta.float().cuda(), c.B, c.P, c.C, c.G, c.eps, c.silu, c.with_y)
    _report(f"{c.name} [{c.plan}]", _check_forward(c.name, d.x, d.gamma, d.beta, c.G, c.silu, got, r, b, c.with_y))


def _tape(r):
    f = lambda t: t.float().double()
    return f(r.mean), f(r.rstd), f(r.scale), f(r.shift)


def _check_backward(tag, x, dy, add, tape, G, silu, d_adds, got):
    adt = _L().act_dtype()
    m = N.backward(x, dy, add, *tape, G, silu)
    bb = N.backward_bound(x, dy, add, *tape, G, silu, m, d_adds, adt)
    dx, k0, k1 = got
    return {"k0": _check(tag + " k0", k0, m.k0, bb.k0), "k1": _check(tag + " k1", k1, m.k1, bb.k1), "dx": _check(tag + " dx", dx, m.dx, bb.dx)}


@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("silu", [0, 1], ids=["lin", "silu"])
@pytest.mark.parametrize("case", N.CASES, ids=repr)
def test_backward_classic(case, silu, with_add):
    c = case
    d, r, _ = _reference(c.name)
    tape = _tape(r)
    add = d.add if with_add else None
    got = _run_backward(_dev16(d.x), _dev16(d.dy), _dev16(add) if with_add else None, *tape, c.B, c.P, c.C, c.G, silu)
    _report(f"{c.name} bwd silu {silu} add {int(with_add)}", _check_backward(c.name, d.x, d.dy, add, tape, c.G, silu, c.bwd_d, got))


@pytest.mark.parametrize("name", N.ROUND_TRIP)
def test_backward_from_the_tape_the_forward_kernel_wrote(name):
    c = BY_NAME[name]
    d, r, b = _reference(name)
    x = _dev16(d.x)
    _, mean, rstd, scale, shift = _run_forward(x, d.gamma.float().cuda(), d.beta.float().cuda(), c.B, c.P, c.C, c.G, c.eps, c.silu, c.with_y)
    tape = (mean, rstd, scale, shift)
    got = _run_backward(x, _dev16(d.dy), _dev16(d.add), *tape, c.B, c.P, c.C, c.G, c.silu)
    _report(f"{name} [{c.plan}] round trip", _check_backward(name, d.x, d.dy, d.add, tape, c.G, c.silu, c.bwd_d, got))


# ------------------------------------------------------------------------------------------------------------- producer route
class _GuardedLib:
    """the library with dmx_groupnorm_part_floats enlarged by the guard: the helpers of the existing tests allocate their NaN-filled
    partial-sum buffer from it, so the buffer they return carries GUARD more elements than the library declares"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, k):
        return getattr(self._lib, k)

    def dmx_groupnorm_part_floats(self, B, P, Nn):
        return self._lib.dmx_groupnorm_part_floats(B, P, Nn) + GUARD


class _GuardedL:
    def __init__(self, L):
        self._L, self._glib = L, _GuardedLib(L.lib())

    def __getattr__(self, k):
        return getattr(self._L, k)

    def lib(self):
        return self._glib


def _check_part(tag, part, B, P, Cc, tm, sums):
    """part: the buffer a producer launch wrote; sums: ((ref, bound), (ref, bound)) per (image, slot, quad)"""
    declared = _L().lib().dmx_groupnorm_part_floats(B, P, Cc)
    assert part.numel() == declared + GUARD
    h = part.cpu().double()
    ns, nq = N.cdiv(P, tm), Cc // 4
    used = B * (ns + 1) * nq * 2
    assert used <= declared
    assert bool(torch.isnan(h[used:]).all()), f"{tag}: partial sums written outside the (image, slot, quad) layout or beyond the declared buffer"
    v = h[:used].view(B, ns + 1, nq, 2)
    assert bool(torch.isnan(v[:, ns]).all()), f"{tag}: the spare slot of an image was written"
    assert bool(torch.isfinite(v[:, :ns]).all()), f"{tag}: a slot was not written"
    (s0, b0), (s1, b1) = sums
    return _check(tag + " slot sum 0", v[:, :ns, :, 0], s0, b0), _check(tag + " slot sum 1", v[:, :ns, :, 1], s1, b1)


def _affine(name, Cc):
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    return (1.0 + 0.3 * torch.randn(Cc, generator=g)).double(), (0.2 * torch.randn(Cc, generator=g)).double()


def _parts_forward(tag, x, regions, chains, G, silu):
    """x (B, P, C) on the device, regions for the entry point, chains = [(tm, slots, quads per group)] for adds(): statistics only and with y"""
    adt = _L().act_dtype()
    B, P, Cc = x.shape
    gamma, beta = _affine(tag, Cc)
    xd = x.cpu().double()
    w = {}
    for with_y in (False, True):
        pl = N.parts_plan(P, Cc, with_y, [(tm, Pr, nq) for _, tm, Pr, nq, _, _ in regions])
        d = N.adds(pl, P, Cc, G, regions=chains)
        r = N.forward(xd, gamma, beta, G, 1e-5, silu, with_y=with_y)
        b = N.forward_bound(xd, gamma, beta, G, 1e-5, silu, r, d, False, adt, with_y=with_y)
        got = _run_forward(x, gamma.float().cuda(), beta.float().cuda(), B, P, Cc, G, 1e-5, silu, with_y, parts=regions)
        for k, v in _check_forward(f"{tag} [{pl}]", xd, gamma, beta, G, silu, got, r, b, with_y).items():
            w[f"{k}/{pl[6:]}"] = v
    return w


@pytest.mark.parametrize("entry", N.PRODUCER, ids=lambda e: e[0])
def test_producer_forward(entry):
    """EPI_GNSTATS: the partial sums themselves, then the GroupNorm that combines them (both plans of the producer entry)"""
    name, cfg, B, P, K, Cc, G, silu = entry
    g = torch.Generator().manual_seed(P + Cc + cfg)
    x, part, tm = _produce(_GuardedL(_L()), g, B, P, K, Cc, cfg)
    x = x.contiguous()
    s = _check_part(name, part, B, P, Cc, tm, N.forward_slots(x.cpu().double(), tm))
    w = {"sum v": s[0], "sum v^2": s[1]}
    w.update(_parts_forward(name, x, [(part, tm, P, Cc // 4, 0, Cc // 4)], [(tm, N.cdiv(P, tm), N.cdiv(Cc // G, 4))], G, silu))
    _report(f"{name} tm {tm}", w)


def test_producer_forward_concatenation_seam_inside_a_group():
    """64 + 96 channels in 8 groups of 20: group 3 (channels 60 .. 79) straddles the seam"""
    B, P, K, Ca, Cb, G = 3, 1000, 64, 64, 96, 8
    g = torch.Generator().manual_seed(8)
    Lg = _GuardedL(_L())
    a, pa, tma = _produce(Lg, g, B, P, K, Ca)
    b, pb, tmb = _produce(Lg, g, B, P, K, Cb)
    w = {}
    for nm, t, pt, tm, Cs in (("a", a, pa, tma, Ca), ("b", b, pb, tmb, Cb)):
        s = _check_part(f"seam {nm}", pt, B, P, Cs, tm, N.forward_slots(t.contiguous().cpu().double(), tm))
        w[f"sum v/{nm}"], w[f"sum v^2/{nm}"] = s
    x = torch.cat([a, b], dim=2).contiguous()
    w.update(_parts_forward("prod-seam", x, [(pa, tma, P, Ca // 4, 0, Ca // 4), (pb, tmb, P, Cb // 4, Ca // 4, Cb // 4)],
                            [(tma, N.cdiv(P, tma), 5), (tmb, N.cdiv(P, tmb), 5)], G, 0))
    _report("prod-seam", w)


def test_producer_forward_four_parity_regions():
    """an upsample-folded convolution at 8 x 12 -> 16 x 24: four launches over the 96 low-resolution positions of an image, one per output
    parity; output pixel (2 y + py, 2 x + px) comes from launch 2 py + px"""
    B, H, W, K, Cc, G = 3, 8, 12, 64, 64, 8
    g = torch.Generator().manual_seed(7)
    Lg = _GuardedL(_L())
    q = [_produce(Lg, g, B, H * W, K, Cc) for _ in range(4)]
    full = torch.empty(B, 2 * H, 2 * W, Cc, dtype=q[0][0].dtype, device="cuda")
    w = {}
    for i, (t, pt, tm) in enumerate(q):
        full[:, i // 2::2, i % 2::2] = t.reshape(B, H, W, Cc)
        s = _check_part(f"parity {i}", pt, B, H * W, Cc, tm, N.forward_slots(t.contiguous().cpu().double(), tm))
        w[f"sum v/{i}"], w[f"sum v^2/{i}"] = s
    x = full.reshape(B, 4 * H * W, Cc).contiguous()
    w.update(_parts_forward("prod-parity", x, [(pt, tm, H * W, Cc // 4, 0, Cc // 4) for _, pt, tm in q],
                            [(tm, N.cdiv(H * W, tm), 2) for _, _, tm in q], G, 1))
    _report("prod-parity", w)


@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("entry", N.PRODUCER, ids=lambda e: e[0])
def test_producer_backward(entry, with_add):
    """EPI_GNBWD: the two backward sums per (image, slot, quad) against float64 sums over the stored dy and x (the tape is the one the
    forward kernel wrote: an input here), then k0 / k1 / dx from them against the closed form"""
    name, cfg, B, P, K, Cc, G, silu = entry
    L, adt = _L(), _L().act_dtype()
    g = torch.Generator().manual_seed(11 * P + Cc + cfg)
    xd = (0.6 + 1.7 * torch.randn(B, P, Cc, generator=g, dtype=torch.float64)).to(adt)
    x = xd.cuda()
    xd = xd.double()
    gamma, beta = _affine(name, Cc)
    dy, part, tm, (stats, scale, shift, _) = _forward_and_dgrad(_GuardedL(L), g, x, gamma.float().cuda(), beta.float().cuda(), G, silu, K, cfg)
    dy = dy.contiguous()
    st = stats.cpu().double()
    tape = (st[..., 0], st[..., 1], scale.cpu().double(), shift.cpu().double())
    dyd = dy.cpu().double()
    m = N.backward(xd, dyd, None, *tape, G, silu)
    s = _check_part(name, part, B, P, Cc, tm, N.backward_slots(xd, dyd, tape[2], tape[3], m, silu, tm))
    w = {"sum dxh": s[0], "sum dxh (x - mean)": s[1]}
    add = torch.randn(B, P, Cc, generator=g).to(adt) if with_add else None
    got = _run_backward(x, dy, add.cuda() if with_add else None, *tape, B, P, Cc, G, silu, parts=[(part, tm, P, Cc // 4, 0, Cc // 4)])
    d = N.adds("parts_stats", P, Cc, G, regions=[(tm, N.cdiv(P, tm), N.cdiv(Cc // G, 4))])
    w.update(_check_backward(name, xd, dyd, add.double() if with_add else None, tape, G, silu, d, got))
    _report(f"{name} bwd tm {tm} add {int(with_add)}", w)


@pytest.mark.parametrize("Cc,G,why", [(36, 4, "C % 8"), (40, 16, "C % G"), (96, 48, "G = 48"), (256, 128, "G = 128"), (2056, 8, "C = 2056")])
def test_refusals_leave_every_output_untouched(Cc, G, why):
    L, adt = _L(), _L().act_dtype()
    B, P = 2, 16
    x = torch.zeros(B, P, Cc, dtype=adt, device="cuda")
    gamma, beta = torch.ones(Cc, device="cuda"), torch.zeros(Cc, device="cuda")
    ybuf, dxbuf = _sent16(B * P * Cc), _sent16(B * P * Cc)
    f32 = {k: _nan(n) for k, n in (("stats", B * 64 * 2), ("scale", B * Cc), ("shift", B * Cc), ("k0", B * Cc), ("k1", B * Cc), ("partial", B * 512 * 64 * 2))}
    tape = {k: torch.ones(n, device="cuda") for k, n in (("stats", B * 64 * 2), ("scale", B * Cc), ("shift", B * Cc))}
    rc = L.lib().dmx_groupnorm_raw(_p(x), _p(ybuf), _p(gamma), _p(beta), _p(f32["stats"]), _p(f32["scale"]), _p(f32["shift"]), _p(f32["partial"]),
                                   B, P, Cc, G, 1e-5, 1, _stream())
    assert rc != 0, f"forward accepted {why}"
    rc = L.lib().dmx_groupnorm_bwd_raw(_p(x), _p(x), None, _p(dxbuf), _p(tape["stats"]), _p(tape["scale"]), _p(tape["shift"]), _p(f32["k0"]), _p(f32["k1"]),
                                       _p(f32["partial"]), B, P, Cc, G, 1, 0, None, None, _stream())
    assert rc != 0, f"backward accepted {why}"
    torch.cuda.synchronize()
    assert bool((ybuf == N.SENT16).all()) and bool((dxbuf == N.SENT16).all()), why
    for k, t in f32.items():
        assert bool(torch.isnan(t).all()), f"{why}: {k} was written"
