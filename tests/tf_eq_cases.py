"""Shared by tests/test_tf_eq_bound_host.py (CPU) and tests/test_gpu_blind_eq.py (GPU): float64 models of the curve gradient and of the
update of the blind equalisation (csrc/tf_eq.hip), the element-wise bound of the gradient, an fp32 emulation in
the kernel's documented order, mutants and the case table.  Written the way tests/tf_gain_cases.py is; no GPU dependency.

MODEL (float64, from the definition; `model_wgrad`): n_fft = 1024, hop = 256, periodic Hann w, x and u = dy taken as zero outside [0, L)
    frames     t = 0 .. T - 1, T = ceil(L / 256) + 3; frame t covers the samples s = (t - 3) 256 + n, n = 0 .. 1023
    analysis   X[k, t] = sum_n w[n] x[s] exp(-2 pi i k n / 1024), U[k, t] the same of u, k = 0 .. 512
    gradient   dg[k] = (h_k / (c 1024)) sum_t Re(X[k, t] conj(U[k, t])), h_0 = h_512 = 1, else 2, c = 1.5
`model_apply` is A_g(x) = (1 / c) P^T W F^-1 diag(g) F W P x in float64 and `model_update` the update lines of the issue, per clip.

BOUND on part.sum(1), from the number formats alone (u = 2^-24, gamma(n) = n u / (1 - n u); `bound`), a componentwise absolute-value
propagation of the model; every line is one line of `bound`.  C_IN and C_FFT are those of spectral_cases.py (same FFT code,
csrc/fft1024.h).  The kernel runs two real transforms per frame (the form that was built), not the packed complex one.
    frames     x_n = w_n x_s and u_n = w_n u_s carry C_IN = 3 roundings each (window table, product; the third is unused here and kept so
               that the constant is the same)
    forward    |dX_k| <= (C_FFT + C_IN) u Sx_t =: bX, Sx_t = sum_n |w_n x_s|;  |dU_k| <= (C_FFT + C_IN) u Su_t =: bU  (moduli of the
               complex errors; every path from a sample to a bin has modulus one)
    bilinear   p = Re(X conj(U)) = Xr Ur + Xi Ui: |Re(a conj(b))| <= |a| |b| gives the input part |X| bU + |U| bX + bX bU; the two
               products and their sum are one rounding each, two deep: gamma(2) (|X| + bX) (|U| + bU)
               b(p) = |X| bU + |U| bX + bX bU + gamma(2) (|X| + bX) (|U| + bU)
    sums       a wave's accumulator adds its ceil(SEG / 4) = 4 frames of a segment, three more additions combine the four waves (counted
               as 4), and S rows are added per clip: sum_t b(p) + gamma(4 + 4 + S) sum_t (|p| + b(p))
    scale      fp32(1 / 1536) and the product, two roundings (h_k = 2 is exact): together gamma(4 + 4 + S + 2)
               b(dg_k) = (h_k / 1536) [sum_t b(p) + gamma(10 + S) sum_t (|p| + b(p))]
The kernel is bilinear and has no gates: no ambiguous elements, no cap -- EVERY element must lie within the bound, and where u = 0 the
bound is zero: the kernel must give exactly zero there (the tests ask for +0.0).  The bound holds with or without FMA contraction.

EMULATION (`emulate`): numpy float32 in the kernel's order -- segments of SEG frames; frame t of a segment into accumulator
(t - t0) % 4 in increasing t, the accumulators summed ((a0 + a1) + a2) + a3, times fp32(1 / 1536), times h_k; -> part (B, S, 513).
`total` adds the rows in segment order in fp32, as eq_update does.  It validates the bound on the CPU and carries the mutants of the
segment / wave logic.  It is not a second oracle.

MUTANTS: `MUTANTS` maps a name to (where it lives, case names); each must leave the bound in at least one element of one listed case.
The issue's "mirror index 1023 - k" belongs to the packed form, which was not built, and has no counterpart here.

CASES: see `CASES`; every case carries `why`, the branch it is there for."""
from types import SimpleNamespace

import numpy as np

from tests import spectral_cases as S

U, C_IN, C_FFT, gamma, ratio = S.U, S.C_IN, S.C_FFT, S.gamma, S.ratio
f32, f64 = np.float32, np.float64
NF, HOP, NB, HALO = 1024, 256, 513, 3
SEG = 16
C_OLA = 1.5
SCALE = 1.0 / (C_OLA * NF)


def frames(L):
    return -(-L // HOP) + HALO


def segments(L):
    return -(-frames(L) // SEG)


def herm():
    h = np.full(NB, 2.0)
    h[0] = h[NB - 1] = 1.0
    return h


# ------------------------------------------------------------------------------------------------------------------ cases and inputs
def _case(name, why, L, B=2, stride_x=None, stride_dy=None, x="sine", dy="noise"):
    return SimpleNamespace(name=name, why=why, L=L, T=frames(L), S=segments(L), B=B, stride_x=stride_x or L, stride_dy=stride_dy or L, x=x, dy=dy)


def _cases():
    out = []
    for L, why in ((300, "shorter than a frame (T = 5)"), (1024, "one frame length"), (1025, "one frame length + 1"),
                   (3328, "T = 16: exactly one segment"), (3329, "T = 17: a second segment of one frame"), (4999, "odd length, two segments"),
                   (6400, "a multiple of the hop; the step tests' length"), (9000, "T = 39: three segments, the last ragged")):
        out.append(_case(f"L{L}", why, L, B=3 if L in (300, 3329) else 2))
    out.append(_case("L6400_stride", "row strides larger than L: 6432 for x, 6416 for dy", 6400, stride_x=6432, stride_dy=6416))
    out.append(_case("L4999_edge", "-0.0f and a large-magnitude sample, in x and in dy", 4999, x="edge", dy="edge"))
    out.append(_case("L3329_impulse_first", "dy a single impulse at sample 0", 3329, dy="impulse_first"))
    out.append(_case("L3329_impulse_last", "dy a single impulse at sample L - 1 = 3328: position 0 of frame T - 1, where the window is zero",
                     3329, dy="impulse_last"))
    out.append(_case("L300_impulse_last", "dy a single impulse at sample L - 1 = 299: position 43 of frame T - 1", 300, dy="impulse_last"))
    for k in (0, 1, 511, 512):
        out.append(_case(f"L3329_tone{k}", f"x a pure tone on bin {k}", 3329, x=f"tone{k}"))
    out.append(_case("L4999_dy_zero", "dy == 0: exactly +0.0 everywhere", 4999, B=3, dy="zero"))
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}


_INPUTS = {}


def inputs(c):
    """everything a case feeds the kernel, fp32 numpy, identical on the host and the GPU side; cached and never modified"""
    if c.name in _INPUTS:
        return _INPUTS[c.name]
    xs = S._clips("eq/" + c.name, "x", c.B, c.stride_x).copy()            # sine plus noise; the last clip pure noise
    ds = (S._clips("eq/" + c.name, "dy", c.B, c.stride_dy)[::-1] * f32(0.05)).copy()   # the FIRST clip pure noise; a cotangent is small
    L = c.L
    if c.x == "edge":
        xs[:, 17] = f32(-0.0)
        xs[:, 100:104] = f32(-0.0)
        xs[0, 2500] = f32(3.0e4)
        xs[1, L - 1] = f32(-1.0e3)
    elif c.x.startswith("tone"):
        k = int(c.x[4:])
        xs[:] = np.cos(2.0 * np.pi * k * np.arange(c.stride_x) / NF).astype(f32) * f32(0.5)
    if c.dy == "edge":
        ds[:, 33] = f32(-0.0)
        ds[1, 1200] = f32(-2.0e3)
    elif c.dy in ("impulse_first", "impulse_last"):
        ds[:] = 0
        ds[:, 0 if c.dy == "impulse_first" else L - 1] = np.linspace(1.0, 2.0, c.B).astype(f32)
    elif c.dy == "zero":
        ds[:] = 0
    i = SimpleNamespace(x_store=xs, dy_store=ds, x=xs[:, :L], dy=ds[:, :L])
    _INPUTS[c.name] = i
    return i


# ------------------------------------------------------------------------------------------------------------------ float64 model
def window():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NF) / NF)


def frame_index(L, T, mut=None):
    """(T, 1024) sample index of position n of frame t (outside [0, L): the zero extension)"""
    return (np.arange(T)[:, None] - (2 if mut == "frame_offset_2" else HALO)) * HOP + np.arange(NF)[None]


def _framed(x, L, s, win):
    inside = (s >= 0) & (s < L)
    return np.where(inside[None], x[:, np.clip(s, 0, L - 1)], x.dtype.type(0)) * win


def model_wgrad(x, dy, L, mut=None):
    """float64 dg: x, dy (B, >= L) -> namespace with every intermediate; r.dg (B, 513)"""
    x, dy = np.asarray(x, f64)[:, :L], np.asarray(dy, f64)[:, :L]
    if mut == "dy_of_clip_0":
        dy = np.broadcast_to(dy[:1], dy.shape)
    T = frames(L)
    r = SimpleNamespace(T=T, S=segments(L))
    r.s = frame_index(L, T, mut)
    win = window()
    r.xw, r.uw = _framed(x, L, r.s, win), _framed(dy, L, r.s, win)
    r.X, r.U = np.fft.rfft(r.xw, axis=-1), np.fft.rfft(r.uw, axis=-1)                 # (B, T, 513)
    r.p = (r.X * r.U).real if mut == "no_conjugate" else (r.X * np.conj(r.U)).real
    if mut == "frame_last_skipped":
        r.p[:, T - 1] = 0.0
    h = np.full(NB, 2.0) if mut == "h2_at_dc_and_nyquist" else herm()
    r.dg = r.p.sum(1) * h * (1.0 / NF if mut == "no_inv_c" else SCALE)
    return r


def bound(r):
    """element-wise bound (B, 513) on |part.sum(1) - model| for the model run r"""
    bX = (C_FFT + C_IN) * U * np.abs(r.xw).sum(-1, keepdims=True)
    bU = (C_FFT + C_IN) * U * np.abs(r.uw).sum(-1, keepdims=True)
    aX, aU = np.abs(r.X), np.abs(r.U)
    bp = aX * bU + aU * bX + bX * bU + gamma(2) * (aX + bX) * (aU + bU)
    sb, sa = bp.sum(1), np.abs(r.p).sum(1)
    return herm() * SCALE * (sb + gamma(4 + 4 + r.S + 2) * (sa + sb))


def model_apply(x, g, L):
    """float64 A_g(x): x (B, >= L), g (513,) or (B, 513) -> (B, L)"""
    x = np.asarray(x, f64)[:, :L]
    B, T = x.shape[0], frames(L)
    s, win = frame_index(L, T), window()
    inside = (s >= 0) & (s < L)
    Y = np.fft.rfft(_framed(x, L, s, win), axis=-1) * np.broadcast_to(np.asarray(g, f64), (B, NB))[:, None, :]
    wf = np.fft.irfft(Y, n=NF, axis=-1) * win
    y = np.zeros((B, L))
    for b in range(B):
        np.add.at(y[b], s[inside], wf[b][inside])
    return y / C_OLA


def model_update(dg, g, m, v, k, lr=0.05, b1=0.9, b2=0.999, eps=1e-8, peak=True):
    """The update lines of the issue in float64, per clip: (B, 513) each -> (g', m', v'); a clip with a non-finite dg or g~, or with
    max g~ == 0 under the peak normalisation, is returned unchanged."""
    dg, g, m, v = (np.asarray(a, f64) for a in (dg, g, m, v))
    with np.errstate(all="ignore"):
        mn = b1 * m + (1 - b1) * dg
        vn = b2 * v + (1 - b2) * dg * dg
        step = g - lr * (mn / (1 - b1 ** k)) / (np.sqrt(vn / (1 - b2 ** k)) + eps)
        gt = np.where(step > 0, step, np.where(np.isnan(step), step, 0.0))
        top = np.max(np.where(np.isnan(gt), -np.inf, gt), axis=1, keepdims=True)
        keep = ~(np.isfinite(dg).all(1, keepdims=True) & np.isfinite(gt).all(1, keepdims=True))
        if peak:
            keep = keep | ~(top > 0)
            gt = gt / np.where(top > 0, top, 1.0)
    return np.where(keep, g, gt), np.where(keep, m, mn), np.where(keep, v, vn)


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation
def emulate(x, dy, L, mut=None):
    """fp32 emulation of tf_wgrad_kernel -> part (B, S, 513) float32"""
    x, dy = np.asarray(x, f32)[:, :L], np.asarray(dy, f32)[:, :L]
    B, T, nseg = x.shape[0], frames(L), segments(L)
    win = window().astype(f32)
    s = frame_index(L, T)
    xw, uw = _framed(x, L, s, win), _framed(dy, L, s, win)
    Xr, Xi = S._fft1024(xw, np.zeros_like(xw), False)
    Ur, Ui = S._fft1024(uw, np.zeros_like(uw), False)
    p = Xr[..., :NB] * Ur[..., :NB] + Xi[..., :NB] * Ui[..., :NB]                      # (B, T, 513), every operation rounded to fp32
    h = herm().astype(f32)
    part = np.zeros((B, nseg, NB), f32)
    for seg in range(nseg):
        t0, t1 = seg * SEG, min(seg * SEG + SEG, T)
        last = t1 + 1 if mut == "segment_first_frame_twice" and t1 < T else t1        # the neighbour's first frame as well
        acc = np.zeros((4, B, NB), f32)
        for t in range(t0, last):
            w = (t - t0) % 4
            if mut == "fourth_wave_dropped" and w == 3:
                continue
            acc[w] = acc[w] + p[:, t]
        tot = ((acc[0] + acc[1]) + acc[2]) + acc[3]
        part[:, seg] = (tot * f32(1.0 / 1536.0)) * h
    return part


def total(part):
    """the rows added in segment order in fp32, as eq_update_kernel does: (B, S, 513) -> (B, 513) float32"""
    part = np.asarray(part, f32)
    d = np.zeros((part.shape[0], part.shape[2]), f32)
    for seg in range(part.shape[1]):
        d = d + part[:, seg]
    return d


# ------------------------------------------------------------------------------------------------------------------ mutants
# name -> (where: "model" or "emulation", case names).  Every listed case is run; the mutant must leave the bound in at least one.
MUTANTS = {
    "h2_at_dc_and_nyquist": ("model", ["L3329_tone0", "L3329_tone512"]),
    "no_inv_c": ("model", ["L1024", "L6400"]),
    "frame_offset_2": ("model", ["L6400", "L300"]),
    "frame_last_skipped": ("model", ["L300_impulse_last", "L4999", "L300"]),
    "fourth_wave_dropped": ("emulation", ["L1024", "L9000"]),
    "segment_first_frame_twice": ("emulation", ["L4999", "L9000"]),
    "dy_of_clip_0": ("model", ["L300", "L3329"]),
    "no_conjugate": ("model", ["L1025", "L3329_tone1"]),
}


_RUNS = {}


def reference(c):
    """(model run, bound) of a case: computed once, shared, never modified"""
    if c.name not in _RUNS:
        i = inputs(c)
        r = model_wgrad(i.x, i.dy, c.L)
        _RUNS[c.name] = (r, bound(r))
    return _RUNS[c.name]


def run_case(c, mut=None, where=None):
    """largest |got - model| / bound of the emulation, or of a mutated model / emulation"""
    i = inputs(c)
    r, q = reference(c)
    if where == "model":
        got = model_wgrad(i.x, i.dy, c.L, mut).dg
    else:
        got = total(emulate(i.x, i.dy, c.L, mut if where == "emulation" else None))
    return ratio(got, r.dg, q)


# ------------------------------------------------------------------------------------------------------------------ recovery loop
def recovery_inputs(L=6400, B=2, seed=5):
    """The recovery test's own inputs, fp32 numpy: x = 0.1 randn (B, L) and the true curve, lowpass_curve(16000, 1500, 4) with the bins from
    300 up set to zero (the clamp at zero is exercised), peak 1."""
    from diffmusic_amd.inverse_problem import dsp
    x = (0.1 * np.random.default_rng(seed).standard_normal((B, L))).astype(f32)
    true = dsp.lowpass_curve(16000, 1500.0, 4).copy()
    true[300:] = 0.0
    return x, (true / true.max()).astype(f32)


def recovery_loop(x, true, L, steps=200, lr=0.05, b1=0.9, b2=0.999, eps=1e-8):
    """float64 restatement of `steps` wav_form guidance calls of BlindEqualizationOperator(init="flat", normalize="peak") on the fixed x:
    -> relative L2 error of the estimate per clip before every step and after the last, (steps + 1, B)."""
    x64 = np.asarray(x, f64)[:, :L]
    B = x64.shape[0]
    tr = np.broadcast_to(np.asarray(true, f64), (B, NB))
    y = model_apply(x64, tr, L)
    g, m, v = np.ones((B, NB)), np.zeros((B, NB)), np.zeros((B, NB))
    errs = []
    for k in range(1, steps + 1):
        errs.append(np.linalg.norm(g - tr, axis=1) / np.linalg.norm(tr, axis=1))
        res = y - model_apply(x64, g, L)
        dy = -res / np.linalg.norm(res, axis=1, keepdims=True)                         # d ||y - A_g x|| / d (A_g x)
        dg = model_wgrad(x64, dy, L).dg
        g, m, v = model_update(dg, g, m, v, k, lr, b1, b2, eps, True)
    errs.append(np.linalg.norm(g - tr, axis=1) / np.linalg.norm(tr, axis=1))
    return np.stack(errs)
