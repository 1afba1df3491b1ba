"""Shared by tests/test_mdct_bound_host.py (CPU) and tests/test_gpu_codec.py (GPU): a float64 model of the MDCT quantiser
(csrc/mdct_quant.hip), its element-wise bound, an fp32 emulation in the kernel's documented order, mutants and the
case table.  Written the way tests/tf_gain_cases.py is; no GPU dependency.

MODEL (float64, from the definition; `analysis`, `quantise`, `synthesis`): N = 512, frame length 1024, hop 512, x zero outside [0, L)
    frames     t = 0 .. T - 1, T = ceil(L / 512) + 1; frame t covers the samples s = (t - 1) 512 + n, n = 0 .. 1023
    analysis   C[k, t] = sqrt(2 / N) sum_n w[n] x[s] cos(pi / N (n + 1/2 + N / 2)(k + 1/2)), w[n] = sin(pi (n + 1/2) / 1024)
    map        QUANT: q = rint(C / D) half-even, f = q D; D = 0 -> f = C, D = inf -> f = 0 (code 0); |C / D| >= 2^23 -> f = C; MARK = INT32_MIN
               PASS: f = C where D < inf, else 0.     PROJECT: f = clamp(C, (q - 1/2) D, (q + 1/2) D) on whole frames where 0 < D < inf, q coded
    synthesis  A(x)[s] = sum_{t covers s} sqrt(2 / N) w[n] sum_k f[k, t] cos(...)

THE GATE.  The quantiser is a gate on every coefficient, so the comparison has two steps.
    codes      a coefficient is AMBIGUOUS when its float64 C / D lies within m = bC / D + 2 u |C / D| of a half-integer (bC: the coefficient
               bound below; the second term the rounding of the division) or of the 2^23 limit.  The kernel's code must EQUAL the model's on
               every unambiguous coefficient and be one of the two integers next to C / D on an ambiguous one.  At most AMBIG_CAP = 2 % of a
               case's coefficients may be ambiguous; `STEP_CASES` (what the step tests build on) must have none.
    waveform   EVERY element is then compared with the model synthesised from the kernel's OWN codes (`values_from_codes`), under the
               synthesis bound.  No sample is left out.

BOUND, from the number formats alone (u = 2^-24, gamma(n) = n u / (1 - n u)); every line is one line of the kernel's arithmetic.  C_IN and
C_FFT are those of spectral_cases.py (same FFT code, csrc/fft1024.h).
    frame      xw = w_n x_s: C_IN = 3 roundings -- window table, product, and the table of the pre-twiddle exp(-i pi n / 1024); the product
               with the pre-twiddle is a fourth: |du_n| <= gamma(C_IN + 1) |w_n x_s| (modulus of the complex error)
    forward    |dU_k| <= (C_FFT + C_IN + 1) u S_t, S_t = sum_n |w_n x_s| (every path from u_n to U_k has modulus one)
    post       c = Re(U_k post_k) / 16: post table, two products and a subtraction, each at most u |U_k| (|post_k| = 1, Cauchy-Schwarz);
               1 / 16 = sqrt(2 / 512) is a power of two (exact):  bC = [bU + 3 u (|U_k| + bU)] / 16
    map        coded: f = q D, one rounding, b(f) = u |q D|; passed through (MARK): b(f) = bC; discarded: 0.  PASS: bC where kept.
               PROJECT: clamp is 1-Lipschitz in all three arguments and (q -+ 1/2) is exact: b(f) = max(bC, u |lo|, u |hi|)
    Z          Z_k = f conj(post_k): table and product, b(Z) = b(f) + 2 u (|f| + b(f))
    inverse    over the 512 non-zero bins, modulus of the complex error: b(z_n) = sum_k b(Z_k) + C_FFT u sum_k (|Z_k| + b(Z_k))
    pre        g = Re(z_n conj(pre_n)) / 16: table, two products, an addition: b(g) = [b(z) + 3 u (|z_n| + b(z))] / 16
    window     two roundings (table, product): b(w g) = w b(g) + 2 u w (|g| + b(g))
    OLA        each accumulator receives one term (0 + a is exact), acc0 + acc1 is one rounding: b(y) = sum_t b + u sum_t (|w g| + b)
A dead sample (both frames discarded) has bound 0 and must be exactly +0.0f.  The bound holds with or without FMA contraction.

EMULATION (`emulate`): numpy float32 in the kernel's order -- slabs of 8 output hops, frames h0 .. h1 of a slab, frame t into accumulator
t & 1.  It validates the bound and the code rule on the CPU, carries the mutants of the slab / frame-range / step-addressing logic and
plants the exact tie.  It is not a second oracle.

MUTANTS: `MUTANTS` maps a name to (where it lives, mode, case names); each must leave the bound or break the code rule in a listed case.

CASES: see `CASES`; B = 2 everywhere; every case carries `why`, the branch it is there for."""
import zlib
from types import SimpleNamespace

import numpy as np

from tests import spectral_cases as S

U, C_IN, C_FFT, gamma, ratio = S.U, S.C_IN, S.C_FFT, S.gamma, S.ratio
f32, f64 = np.float32, np.float64
N, NF = 512, 1024
SLAB_HOPS = 8
SLAB = SLAB_HOPS * N
MARK = -2 ** 31
Q_LIMIT = 2.0 ** 23
AMBIG_CAP = 0.02
QUANT, PASS, PROJECT = "quant", "pass", "project"
MODES = (QUANT, PASS, PROJECT)
N0 = 0.5 + N / 2


def frames(L):
    return -(-L // N) + 1


# ------------------------------------------------------------------------------------------------------------------ cases and inputs
def _case(name, why, L, step, per_clip=False, B=2, full=None, stride=None, out_stride=None, signal="sine"):
    full = full or L
    return SimpleNamespace(name=name, why=why, L=L, T=frames(L), step=step, per_clip=per_clip, B=B, full=full, stride=stride or full,
                           out_stride=out_stride or full, signal=signal)


def _cases():
    out = []
    for L, why in ((300, "shorter than a frame (T = 2)"), (512, "one hop"), (513, "one hop + 1"), (1024, "one frame length"),
                   (SLAB, "exactly one slab"), (SLAB + 1, "one slab + 1: a second slab of one sample"),
                   (4999, "odd length, three hops past one slab"), (6400, "the step tests' length")):
        out.append(_case(f"L{L}_zero", why + "; D = 0: transparent, the identity under the bound", L, "zero"))
        out.append(_case(f"L{L}_rand", why + "; random steps in [0.02, 0.3], shared", L, "rand"))
        out.append(_case(f"L{L}_rand_pc", why + "; random steps, one grid per clip", L, "rand", per_clip=True))
    out.append(_case("L6400_lowpass", "+inf above coefficient 256: the codec's low-pass", 6400, "lowpass"))
    out.append(_case("L6400_lowpass_pc", "+inf above coefficient 256, per clip", 6400, "lowpass", per_clip=True))
    for k in (0, 1, 510, 511):
        out.append(_case(f"L4097_coef{k}", f"a single kept coefficient, k = {k}", SLAB + 1, f"coef{k}", per_clip=(k in (1, 511))))
    for L in (300, 4999):
        out.append(_case(f"L{L}_frame_first", "a single quantised frame at t = 0, the others transparent", L, "frame_first"))
        out.append(_case(f"L{L}_frame_last", "a single quantised frame at t = T - 1", L, "frame_last", per_clip=True))
    out.append(_case("L4999_frame_edge", "a single quantised frame across the slab edge (t = 8: computed by slab 0 as halo and by slab 1)",
                     4999, "frame_edge"))
    out.append(_case("L4999_frame_edge_pc", "the same, per clip", 4999, "frame_edge", per_clip=True))
    out.append(_case("L6400_dead_frames", "frames 6 .. 12 all +inf: samples [3072, 6144) are exactly +0.0f", 6400, "dead_frames"))
    out.append(_case("L6400_dead_frames_pc", "frames 6 .. 12 all +inf, per clip", 6400, "dead_frames", per_clip=True))
    out.append(_case("L6400_stride", "L = 6432 - 32 with row stride 6432; zero tail up to full", 6400, "rand", full=6416, stride=6432, out_stride=6432))
    out.append(_case("L4999_edge", "-0.0f and a large-magnitude sample; steps in [1, 10]", 4999, "coarse", per_clip=True, signal="edge"))
    out.append(_case("L6400_coarse", "steps in [0.5, 1]: what the step tests use; no ambiguous coefficient", 6400, "step_test"))
    out.append(_case("L6400_coarse_lowpass", "the same with +inf above coefficient 256", 6400, "step_test_lowpass"))
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}
STEP_CASES = ("L6400_coarse", "L6400_coarse_lowpass")          # no ambiguous coefficient at all (asserted)


def _rng(name, tag):
    return np.random.default_rng(zlib.crc32(f"mdct/{name}/{tag}".encode()))


def step_test_grid(T, lowpass=False):
    """(512, T) fp32: the fixed grid of the step tests -- 0.5 rising linearly to 1.0 over the coefficients, +inf above 256 with `lowpass`"""
    col = np.linspace(0.5, 1.0, N)
    if lowpass:
        col[256:] = np.inf
    return np.repeat(col.astype(f32)[:, None], T, axis=1)


def _step(c):
    T, n = c.T, (c.B if c.per_clip else 1)
    rng = _rng(c.name, "step")
    rand = rng.uniform(0.02, 0.3, (n, N, T))
    kind = c.step
    if kind == "zero":
        d = np.zeros((n, N, T))
    elif kind == "rand":
        d = rand
    elif kind == "coarse":
        d = rng.uniform(1.0, 10.0, (n, N, T))
    elif kind == "lowpass":
        d = rand.copy()
        d[:, 256:] = np.inf
    elif kind.startswith("coef"):
        d = np.full((n, N, T), np.inf)
        d[:, int(kind[4:])] = rand[:, int(kind[4:])]
    elif kind.startswith("frame_"):
        t = {"frame_first": 0, "frame_last": T - 1, "frame_edge": SLAB_HOPS}[kind]
        d = np.zeros((n, N, T))
        d[:, :, t] = rand[:, :, t]
    elif kind == "dead_frames":
        d = rand.copy()
        d[:, :, 6:13] = np.inf
    elif kind in ("step_test", "step_test_lowpass"):
        d = np.broadcast_to(step_test_grid(T, kind.endswith("lowpass")), (n, N, T))
    else:
        raise KeyError(kind)
    d = np.ascontiguousarray(d).astype(f32)
    return d if c.per_clip else d[0]


_INPUTS = {}


def inputs(c):
    """everything a case feeds the kernel, fp32 numpy, identical on the host and the GPU side; cached and never modified.
    store: the clips with their row stride; x: the L samples; other: a second set of clips (what PROJECT is asked to move)"""
    if c.name in _INPUTS:
        return _INPUTS[c.name]
    store = S._clips("mdct/" + c.name, "rows", c.B, c.stride)         # sine plus noise; the last clip pure noise
    if c.signal == "edge":
        store = store.copy()
        store[:, 17] = f32(-0.0)
        store[:, 100:104] = f32(-0.0)
        store[0, 2500] = f32(1.0e3)
        store[1, c.L - 1] = f32(-1.0e2)
    other = S._clips("mdct/" + c.name, "other", c.B, c.L)
    i = SimpleNamespace(store=store, x=store[:, :c.L], other=other, step=_step(c))
    _INPUTS[c.name] = i
    return i


# ------------------------------------------------------------------------------------------------------------------ float64 model
def window(mut=None):
    n = np.arange(NF, dtype=f64)
    if mut == "hann_symmetric":
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / (NF - 1))
    if mut == "sine_no_half":
        return np.sin(np.pi * n / NF)
    return np.sin(np.pi * (n + 0.5) / NF)


def basis(mut=None):
    """(1024, 512): cos(pi / N (n + n0)(k + 1/2)) sqrt(2 / N), without the window"""
    n, k = np.arange(NF, dtype=f64)[:, None], np.arange(N, dtype=f64)[None]
    return np.sqrt(2.0 / N) * np.cos(np.pi / N * (n + (N / 2 if mut == "phase_no_half" else N0)) * (k + 0.5))


def frame_index(L, T, mut=None):
    """(T, 1024) sample index of position n of frame t (outside [0, L): the zero extension)"""
    return (np.arange(T)[:, None] - (0 if mut == "frame_offset_0" else 1)) * N + np.arange(NF)[None]


def step_btk(D, B, mut=None):
    """(512, T) or (B, 512, T) -> (B, T, 512) float64"""
    D = np.asarray(D, f64)
    if D.ndim == 2:
        D = np.broadcast_to(D, (B,) + D.shape)
    elif mut == "step_of_clip_0":
        D = np.broadcast_to(D[:1], D.shape)
    return D.transpose(0, 2, 1).copy()


def whole_frames(L, T):
    t = np.arange(T)
    return (t >= 1) & (t <= L // N - 1)


def analysis(x, L, mut=None):
    """float64 Phi x: x (B, >= L) -> namespace with s, inside, win, xw (B, T, 1024), C (B, T, 512) and, for the bound, U and S_t"""
    x = np.asarray(x, f64)[:, :L]
    T = frames(L)
    r = SimpleNamespace(T=T, L=L, B=x.shape[0])
    r.s = frame_index(L, T, mut)
    r.inside = (r.s >= 0) & (r.s < L)
    r.win = window(mut)
    r.xw = np.where(r.inside[None], x[:, np.clip(r.s, 0, L - 1)], 0.0) * r.win
    r.C = r.xw @ basis(mut)
    if mut == "no_scale_fwd":
        r.C = r.C / np.sqrt(2.0 / N)
    pre = np.exp(-1j * np.pi * np.arange(NF) / NF)
    r.U = np.fft.fft(r.xw * pre, axis=-1)[..., :N]
    r.S_t = np.abs(r.xw).sum(-1, keepdims=True)
    return r


def analysis_fft(x, L):
    """the FFT route of the kernel in float64: pre-twiddle, FFT, post-twiddle, real part / 16 -> (B, T, 512)"""
    r = analysis(x, L)
    post = np.exp(-1j * np.pi * N0 * (np.arange(N) + 0.5) / N)
    return (r.U * post).real * np.sqrt(2.0 / N)


def quantise(C, D, mut=None):
    """float64 Q: C, D (B, T, 512) -> (codes int64 with MARK, values)"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = C / D
    coded = (D > 0) & np.isfinite(D) & (np.abs(q) < Q_LIMIT)
    rq = np.trunc(np.where(coded, q, 0.0)) if mut == "truncation" else np.rint(np.where(coded, q, 0.0))
    gone = np.isposinf(D)
    codes = np.where(coded, rq, np.where(gone, 0.0, float(MARK))).astype(np.int64)
    f = np.where(coded, rq * np.where(coded, D, 0.0), np.where(gone, 0.0, C))
    return codes, f


def values_from_codes(C, D, codes):
    """the values the kernel's OWN codes stand for: q D where coded, 0 where discarded, the model's C where the kernel passed it through"""
    codes = np.asarray(codes, np.int64)
    marked = codes == MARK
    Df = np.where(np.isfinite(D), D, 0.0)
    return np.where(marked, C, codes.astype(f64) * Df)


def passed(C, D, mut=None):
    return C if mut == "inf_passed" else np.where(np.isposinf(D), 0.0, C)


def cells(D, codes, L, cell=0.5):
    """(lo, hi, active) of PROJECT for the codes (B, T, 512)"""
    codes = np.asarray(codes, np.int64)
    T = D.shape[1]
    active = whole_frames(L, T)[None, :, None] & (D > 0) & np.isfinite(D) & (codes != MARK)
    Df = np.where(active, D, 0.0)
    qf = np.where(active, codes, 0).astype(f64)
    return (qf - cell) * Df, (qf + cell) * Df, active


def projected(C, D, codes, L, mut=None):
    lo, hi, active = cells(D, codes, L, 1.0 if mut == "cell_one" else 0.5)
    return np.where(active, np.minimum(np.maximum(C, lo), hi), C)


def synthesis(r, f, mut=None):
    """float64 Phi^T f for the frames of the analysis run r: f (B, T, 512) -> namespace with Z, z, g, wg, y (B, L)"""
    o = SimpleNamespace()
    if mut == "frame_last_skipped":
        f = f.copy()
        f[:, r.T - 1] = 0.0
    post = np.exp(-1j * np.pi * N0 * (np.arange(N) + 0.5) / N)
    o.Z = f * np.conj(post)
    full = np.concatenate([o.Z, np.zeros_like(o.Z)], axis=-1)
    o.z = np.fft.ifft(full, axis=-1) * NF
    o.g = f @ basis(mut).T
    if mut == "no_scale_inv":
        o.g = o.g / np.sqrt(2.0 / N)
    o.wg = o.g * r.win
    y = np.zeros((r.B, r.L))
    for b in range(r.B):
        np.add.at(y[b], r.s[r.inside], o.wg[b][r.inside])
    o.y = y
    return o


def coef_bound(r):
    """(B, T, 512) bound on |kernel C - model C|"""
    bU = (C_FFT + C_IN + 1) * U * r.S_t * np.ones_like(r.C)
    return (bU + 3 * U * (np.abs(r.U) + bU)) / 16.0


def ambiguous(r, D):
    """-> (mask (B, T, 512), margin in cells): coefficients whose code the formats do not decide"""
    bC = coef_bound(r)
    act = (D > 0) & np.isfinite(D)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = np.where(act, r.C / np.where(act, D, 1.0), 0.0)
        m = np.where(act, bC / np.where(act, D, 1.0), 0.0) + 2 * U * np.abs(q)
    to_half = np.abs(q - np.floor(q) - 0.5)
    amb = act & ((to_half <= m) | (np.abs(np.abs(q) - Q_LIMIT) <= m))
    return amb, m


def code_rule(r, D, codes):
    """-> (number of coefficients that break the code rule, number of ambiguous ones that differ from the model): the kernel's code equals
    the model's on every unambiguous coefficient and is one of the two integers next to C / D on an ambiguous one"""
    codes = np.asarray(codes, np.int64)
    want, _ = quantise(r.C, D)
    amb, _ = ambiguous(r, D)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = np.where(amb, r.C / np.where(amb, D, 1.0), 0.0)
    near = (codes == np.floor(q)) | (codes == np.floor(q) + 1) | ((np.abs(q) > Q_LIMIT / 2) & (codes == MARK))
    bad = np.where(amb, ~near, codes != want)
    return int(bad.sum()), int((amb & (codes != want)).sum())


def synth_bound(r, o, f, bf):
    """element-wise bound (B, L) on |kernel - model| for values f (B, T, 512) that the kernel holds within bf, synthesis run o"""
    bZ = bf + 2 * U * (np.abs(f) + bf)
    bz = bZ.sum(-1, keepdims=True) + C_FFT * U * (np.abs(o.Z) + bZ).sum(-1, keepdims=True)
    bg = (bz + 3 * U * (np.abs(o.z) + bz)) / 16.0
    bwg = r.win * bg + 2 * U * r.win * (np.abs(o.g) + bg)
    sb, sa = np.zeros((r.B, r.L)), np.zeros((r.B, r.L))
    for b in range(r.B):
        np.add.at(sb[b], r.s[r.inside], bwg[b][r.inside])
        np.add.at(sa[b], r.s[r.inside], np.abs(o.wg[b])[r.inside])
    return sb + U * (sa + sb)


def value_bound(r, D, mode, f, codes=None):
    """b(f) of the map: see BOUND"""
    bC = coef_bound(r)
    if mode == QUANT:
        marked = np.asarray(codes, np.int64) == MARK
        return np.where(marked, bC, U * np.abs(f))
    if mode == PASS:
        return np.where(np.isposinf(D), 0.0, bC)
    lo, hi, active = cells(D, codes, r.L)
    return np.where(active, np.maximum(bC, U * np.maximum(np.abs(lo), np.abs(hi))), bC)


def expect(x, D, L, mode, codes=None, mut=None):
    """-> (y (B, L) float64, bound (B, L)) of a mode: QUANT synthesises from `codes` (the kernel's own; None: the model's), PROJECT clamps
    into the cells of `codes`"""
    r = analysis(x, L, mut)
    Db = step_btk(D, r.B, mut)
    if mode == QUANT:
        if codes is None:
            codes, f = quantise(r.C, Db, mut)
        else:
            f = values_from_codes(r.C, Db, codes)
    elif mode == PASS:
        f = passed(r.C, Db, mut)
    else:
        f = projected(r.C, Db, codes, L, mut)
    o = synthesis(r, f, mut)
    return o.y, synth_bound(r, o, f, value_bound(r, Db, mode, f, codes))


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation
def _tables():
    n, k = np.arange(NF, dtype=f64), np.arange(N, dtype=f64)
    pre = np.exp(-1j * np.pi * n / NF)
    post = np.exp(-1j * np.pi * N0 * (k + 0.5) / N)
    return window().astype(f32), pre.real.astype(f32), pre.imag.astype(f32), post.real.astype(f32), post.imag.astype(f32)


def emulate_coeffs(x, L):
    """fp32 C (B, T, 512) in the kernel's order (no FMA)"""
    x = np.asarray(x, f32)[:, :L]
    T = frames(L)
    win, prer, prei, postr, posti = _tables()
    s = frame_index(L, T)
    inside = (s >= 0) & (s < L)
    xw = np.where(inside[None], x[:, np.clip(s, 0, L - 1)], f32(0)) * win
    Ur, Ui = S._fft1024(xw * prer, xw * prei, False)
    return (Ur[..., :N] * postr - Ui[..., :N] * posti) * f32(0.0625)


def emulate_quantise(C, D, mut=None):
    """fp32 Q in the kernel's order -> (codes int64, values fp32)"""
    C, D = np.asarray(C, f32), np.asarray(D, f32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = C / np.where(D > 0, D, f32(1))
        coded = (D > 0) & np.isfinite(D) & (np.abs(q) < f32(Q_LIMIT))
        rq = (np.trunc if mut == "truncation" else np.rint)(np.where(coded, q, f32(0))).astype(f32)
        gone = np.isposinf(D)
        codes = np.where(coded, rq.astype(np.int64), np.where(gone, 0, MARK))
        f = np.where(coded, rq * np.where(coded, D, f32(0)), np.where(gone, f32(0), C)).astype(f32)
    return codes, f


def emulate(x, D, L, mode, codes=None, mut=None):
    """fp32 emulation of csrc/mdct_quant.hip -> (y (B, L) float32, codes (B, T, 512) int64 or None)"""
    x = np.asarray(x, f32)[:, :L]
    B, T, H = x.shape[0], frames(L), -(-L // N)
    D = np.asarray(D, f32)
    if D.ndim == 3 and mut == "step_of_clip_0":
        D = np.broadcast_to(D[:1], D.shape)
    Dt = np.broadcast_to(D, (B,) + D.shape[-2:]).transpose(0, 2, 1)          # (B, T, 512)
    win, prer, prei, postr, posti = _tables()
    C = emulate_coeffs(x, L)
    out_codes = None
    if mode == QUANT:
        out_codes, f = emulate_quantise(C, Dt, mut)
    elif mode == PASS:
        f = np.where(np.isposinf(Dt), f32(0), C)
    else:
        q = np.asarray(codes, np.int64)
        act = whole_frames(L, T)[None, :, None] & (Dt > 0) & np.isfinite(Dt) & (q != MARK)
        qf, Df = np.where(act, q, 0).astype(f32), np.where(act, Dt, f32(0))
        lo, hi = (qf - f32(0.5)) * Df, (qf + f32(0.5)) * Df
        f = np.where(act, np.where(C < lo, lo, np.where(C > hi, hi, C)), C).astype(f32)
    Zr = np.concatenate([f * postr, np.zeros_like(f)], axis=-1)
    Zi = np.concatenate([-(f * posti), np.zeros_like(f)], axis=-1)
    zr, zi = S._fft1024(Zr, Zi, True)
    contrib = ((zr * prer + zi * prei) * f32(0.0625)) * win                    # (B, T, 1024)
    y = np.zeros((B, L), f32)
    n = np.arange(NF)
    for h0 in range(0, H, SLAB_HOPS):
        h1 = min(h0 + SLAB_HOPS, H)
        s0, s1 = h0 * N, min(h1 * N, L)
        t1 = h1 + 1
        if mut == "halo_dropped" and h1 < H:
            t1 -= 1                                                            # the slab's halo frame
        acc = np.zeros((2, B, SLAB), f32)
        for t in range(h0, t1):
            p0 = (t - 1) * N - s0
            ok = (p0 + n >= 0) & (p0 + n < SLAB)
            acc[t & 1][:, p0 + n[ok]] += contrib[:, t, ok]
        y[:, s0:s1] = (acc[0] + acc[1])[:, :s1 - s0]
    return y, out_codes


def plant_tie(C, half, tries=64):
    """For fp32 coefficients C (any shape) find (flat index, step D fp32) with fp32 C / D == half EXACTLY (half = m + 1/2), searching the
    neighbours of fl(C / half) over the first `tries` usable coefficients -> list of (index, D)"""
    flat = np.asarray(C, f32).reshape(-1)
    found = []
    for idx in np.flatnonzero(np.abs(flat) > 1e-3)[:tries]:
        d0 = f32(flat[idx] / f32(half))
        cand = [d0]
        for _ in range(3):
            cand = [np.nextafter(cand[0], f32(0))] + cand + [np.nextafter(cand[-1], f32(np.sign(d0) * np.inf))]
        for d in cand:
            if d > 0 and f32(flat[idx]) / f32(d) == f32(half):
                found.append((int(idx), f32(d)))
                break
    return found


# ------------------------------------------------------------------------------------------------------------------ mutants
# name -> (where: "model" or "emulation", mode, case names).  Every listed case is run; the mutant must fail `check` in at least one.
MUTANTS = {
    "phase_no_half": ("model", QUANT, ["L6400_rand", "L300_zero"]),
    "hann_symmetric": ("model", QUANT, ["L6400_zero", "L300_zero"]),
    "sine_no_half": ("model", QUANT, ["L6400_zero", "L300_zero"]),
    "frame_offset_0": ("model", QUANT, ["L4999_frame_edge", "L300_zero"]),
    "halo_dropped": ("emulation", QUANT, ["L4999_rand", "L4097_zero"]),
    "frame_last_skipped": ("model", QUANT, ["L300_frame_last", "L4999_frame_last", "L6400_zero"]),
    "no_scale_fwd": ("model", QUANT, ["L1024_zero"]),
    "no_scale_inv": ("model", QUANT, ["L1024_zero"]),
    "truncation": ("emulation", QUANT, ["L6400_rand", "L513_rand"]),
    "step_of_clip_0": ("model", QUANT, ["L300_rand_pc", "L4097_coef1"]),
    "inf_passed": ("model", PASS, ["L6400_lowpass", "L4097_coef0"]),
    "cell_one": ("model", PROJECT, ["L6400_rand", "L4999_rand_pc"]),
}


_RUNS = {}


def reference(c):
    """(analysis run, steps (B, T, 512), model codes, ambiguous mask, codes of `other` for PROJECT) of a case: computed once, shared"""
    if c.name not in _RUNS:
        i = inputs(c)
        r = analysis(i.x, c.L)
        Db = step_btk(i.step, c.B)
        codes, _ = quantise(r.C, Db)
        amb, _ = ambiguous(r, Db)
        ocodes, _ = quantise(analysis(i.other, c.L).C, Db)
        _RUNS[c.name] = SimpleNamespace(r=r, D=Db, codes=codes, amb=amb, other_codes=ocodes)
    return _RUNS[c.name]


def check(c, mode, got_y, got_codes=None):
    """-> (largest |got - model| / bound over EVERY element, coefficients that break the code rule, ambiguous coefficients whose code
    differs from the model's).  QUANT: the model is synthesised from got_codes, the kernel's own."""
    i, ref = inputs(c), reference(c)
    broken = differing = 0
    if mode == QUANT:
        broken, differing = code_rule(ref.r, ref.D, got_codes)
        want, bnd = expect(i.x, i.step, c.L, QUANT, codes=got_codes)
    elif mode == PASS:
        want, bnd = expect(i.x, i.step, c.L, PASS)
    else:
        want, bnd = expect(i.x, i.step, c.L, PROJECT, codes=ref.other_codes)
    return ratio(got_y, want, bnd), broken, differing


def run_case(c, mode, mut=None, where=None):
    """`check` of the emulation, or of a mutated model / emulation"""
    i, ref = inputs(c), reference(c)
    pcodes = ref.other_codes if mode == PROJECT else None
    if where == "model":
        r = analysis(i.x, c.L, mut)
        Db = step_btk(i.step, c.B, mut)
        codes = quantise(r.C, Db, mut)[0] if mode == QUANT else None
        y, _ = expect(i.x, i.step, c.L, mode, codes=pcodes if mode == PROJECT else None, mut=mut)
        return check(c, mode, y, codes)
    y, codes = emulate(i.x, i.step, c.L, mode, codes=pcodes, mut=mut if where == "emulation" else None)
    return check(c, mode, y, codes)
