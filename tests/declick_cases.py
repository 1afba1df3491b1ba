"""Shared by tests/test_declick_bound_host.py (CPU) and tests/test_gpu_declick.py (GPU): a float64 model of every stage of the click detector
(csrc/declick.hip), an fp32 emulation in the kernels' documented order, the bounds, the mutants and the case table.
Written the way tests/warp_cases.py and tests/drc_cases.py are; no GPU dependency.

MODEL (float64, from the definition; `model`).  Per clip, y zero outside [0, L), N = 1024, P = 16, F = ceil(L / N).  Frame j, live samples
n in [jN, min(L, (j+1)N)), c of them:

    s[i]  = h[i] y[jN - 512 + i], i = 0 .. 2047, h[i] = 0.5 - 0.5 cos(2 pi i / 2048)
    r[k]  = sum_{i=0}^{2047-k} s[i] s[i+k], k = 0 .. 16
    a     = 0 unless r[0] is a finite positive number, else Levinson-Durbin on (r[0] (1 + 1e-3), r[1], .., r[16])
    e[n]  = y[n] - sum_{i=1}^{16} a[i] y[n-i]
    med   = the |e[n]| of rank ceil(c / 2) (1-based, ascending, NaNs last);  sigma = med / 0.6745f
    flag  = |e[n]| > K (sigma > floor ? sigma : floor);  mask = 0 within `guard` samples of a flag, else 1

The stages are tested TEACHER-FORCED (`check_stages`), so no bound has to survive the threshold:
    r       the op returns r (B, F, 17) beside a, e, sigma and flags -- that is the decision the issue left open -- and it is compared
            element-wise with the model's.  Bound from the number formats (u = 2^-24): the window is w * w with w = sinpif(i / 2048)
            (at most 2 ulp; the argument is exact), so h32 = h (1 + 5u); s = fl(h32 y) adds u; a product of two s 12u; the sum is a chain of
            at most 8 fmaf, a tree of 6 and 2 more additions: |r32 - r| <= gamma(32) sum_i |s_i s_{i+k}| + 4096 * 2^-126 (the last for
            products below the normal range, flushed or not).
    a       against float64 Levinson-Durbin on the SAME fp32 r (the kernel's own).  No element-wise bound was derived; the tolerance per case
            is the fp32 emulation's own largest |a32 - a64| on that case times 8 (fmaf contraction and a different but fixed summation
            order in the kernel).  profiles/declick_parity.json records the emulation's and the kernel's values.
    e       against the float64 filter with the kernel's a: gamma(P + 2) (|y[n]| + sum_i |a_i y[n-i]|) + 2^-126.
    sigma, flags, mask, masked, mask_rows, declick_blend   bit for bit from the kernel's own e, sigma and flags, by their definitions
            (`sigma_from_e`, `flags_from`, `mask_from`, `ref_mask_rows`, `ref_blend`).
    end to end   the kernel's mask against the model's: they may differ only within `guard` of an UNDECIDED sample, one whose model ratio
            |e| / (K max(sigma, floor)) lies in [1 - TAU, 1 + TAU], TAU = 1e-3; a case with more than 1 % undecided samples fails.

EMULATION (`emulate`): numpy float32 in the kernel's order; fmaf(a, b, c) is evaluated in float64 (the product of two fp32 numbers is exact
there) and rounded to fp32; sinpif is the correctly rounded float64 sine.  It validates the bounds on the CPU; it is not a second oracle.

MUTANTS: `MUTANTS` maps a name to (stage, case names); `emulate(..., mutant=name)` must leave the bound or the exact check of that stage on
at least one listed case.

CASES: see `CASES`; every case carries `why`."""
import math
from types import SimpleNamespace

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
N, P, W, LEAD = 1024, 16, 2048, 512
FS = 16000
K_DEF, FLOOR_DEF, GUARD_DEF = 5.0, 1e-5, 3
C_MAD = f32(0.6745)
LOADING = 1e-3
TAU, UNDECIDED_CAP = 1e-3, 0.01
A_FACTOR = 8.0


def gamma(n):
    return n * U / (1.0 - n * U)


def frames(L):
    return -(-L // N)


def live(L, j):
    return min(N, L - j * N)


# ------------------------------------------------------------------------------------------------------------------ inputs
def music(L, seed):
    """12 FM partials in 60 - 4000 Hz plus coloured noise under a 1.5 Hz envelope (float64 -> fp32)."""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(L) / FS
    x = np.zeros(L)
    for _ in range(12):
        fc = math.exp(rng.uniform(math.log(60.0), math.log(4000.0)))
        amp = rng.uniform(0.03, 0.1) / (1.0 + fc / 800.0)
        x += amp * np.sin(2 * np.pi * fc * t + rng.uniform(0.2, 2.0) * np.sin(2 * np.pi * rng.uniform(3.0, 7.0) * t) + rng.uniform(0, 2 * np.pi))
    w = rng.standard_normal(L)
    col = np.empty(L)
    acc = 0.0
    for i in range(L):
        acc = 0.9 * acc + w[i]
        col[i] = acc
    x += 0.004 * col
    x *= 0.6 + 0.4 * np.sin(2 * np.pi * 1.5 * t)
    return x.astype(f32)


def add_clicks(y, seed, count, amp=(0.3, 0.6), max_width=3, at=()):
    """-> (y + clicks, bool array of the click samples): `count` clicks at seeded positions plus one at every position of `at`."""
    rng = np.random.default_rng(2000 + seed)
    L = y.shape[0]
    pos = list(at) + [int(p) for p in rng.integers(0, L, size=max(0, count - len(at)))]
    y = y.copy()
    hit = np.zeros(L, bool)
    for p in pos:
        w = int(rng.integers(1, max_width + 1))
        v = f32(rng.uniform(*amp) * (1 if rng.integers(0, 2) else -1))
        y[p:min(p + w, L)] += v
        hit[p:min(p + w, L)] = True
    return y, hit


def _case(name, why, L, make, K=K_DEF, floor=FLOOR_DEF, guard=GUARD_DEF):
    return SimpleNamespace(name=name, why=why, L=L, make=make, K=K, floor=floor, guard=guard)


def _music_clicks(L, seed, count, **kw):
    return lambda: add_clicks(music(L, seed), seed, count, **kw)[0]


def _noise(L, seed, scale=0.1):
    return lambda: (scale * np.random.default_rng(3000 + seed).standard_normal(L)).astype(f32)


def _set(base, pairs):
    def make():
        y = base().copy()
        for k, v in pairs:
            y[k] = v
        return y
    return make


def _zeros(L):
    return lambda: np.zeros(L, f32)


def _edges_only():
    y = np.zeros(2560, f32)
    y[513:521] = 1.0
    y[2550:2560] = 1.0
    return y


def _silent_inside():
    y = add_clicks(music(5200, 7), 7, 6)[0]
    y[512:3584] = 0.0
    return y


THR_EXACT = f32(K_DEF) * f32(FLOOR_DEF)

CASES = [
    _case("L1", "one sample: one frame, one live sample, the median is that sample", 1, lambda: np.array([0.5], f32)),
    _case("L16", "shorter than the model order plus one", 16, _noise(16, 1)),
    _case("L17", "the first length with a full history", 17, _noise(17, 2)),
    _case("L1023", "one short of a frame", 1023, _music_clicks(1023, 1, 5)),
    _case("L1024", "exactly one frame", 1024, _music_clicks(1024, 2, 5)),
    _case("L1025", "a second frame with one live sample", 1025, _music_clicks(1025, 3, 5, at=(1024,))),
    _case("L1536", "the window's end", 1536, _music_clicks(1536, 4, 8)),
    _case("L2560", "a half last frame, even live count", 2560, _music_clicks(2560, 5, 12)),
    _case("L4133", "five frames, 37 live samples in the last (odd)", 4133, _music_clicks(4133, 6, 20)),
    _case("live999", "odd live count in the last frame", 1024 + 999, _music_clicks(1024 + 999, 8, 10)),
    _case("live1000", "even live count in the last frame: lower and upper median differ", 1024 + 1000, _music_clicks(1024 + 1000, 9, 10)),
    _case("music40", "the issue's input: music with 40 clicks, L = 8229", 8229, _music_clicks(8229, 0, 40)),
    _case("edges", "clicks at n = 0, at L - 1, at 1024 (its guard reaches back over 1023 | 1024) and at 2047 (forward over 2047 | 2048); cut at the clip's ends", 2560,
          lambda: _set(lambda: music(2560, 10), [(0, 0.5), (2559, -0.5), (1024, 0.45), (1500, 0.4), (2047, -0.5)])()),
    _case("merge", "two clicks `guard` apart (their runs merge) and a width-3 burst", 2048,
          lambda: _set(lambda: music(2048, 11), [(600, 0.5), (603, -0.5), (1300, 0.4), (1301, 0.45), (1302, 0.4)])()),
    _case("zeros", "an all-zero clip: r[0] = 0, a = 0, sigma = 0, the floor decides, nothing is flagged", 1536, _zeros(1536)),
    _case("silent_inside", "frames 1 and 2 see only zeros inside a live clip", 5200, _silent_inside),
    _case("silence_click", "digital silence plus one click: a = 0, med = 0, the floor decides", 1536, _set(_zeros(1536), [(700, 0.5)])),
    _case("at_threshold", "one sample exactly AT K * floor in silence: the compare is strict", 1536, _set(_zeros(1536), [(700, THR_EXACT)])),
    _case("dc", "a constant: the autocorrelation is nearly singular, the loading matters", 2048, lambda: np.full(2048, 0.25, f32)),
    _case("sine", "a pure sine: rank 2, the loading matters", 2560,
          lambda: (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(2560) / FS)).astype(f32)),
    _case("square", "a +-1 square of period 50", 2048, lambda: np.where((np.arange(2048) // 25) % 2 == 0, 1.0, -1.0).astype(f32)),
    _case("nan", "one NaN sample: frames 1 and 2 hold it in their windows and fall to a = 0", 4133,
          _set(_music_clicks(4133, 12, 20), [(2000, np.nan)])),
    _case("inf", "one Inf sample", 4133, _set(_music_clicks(4133, 13, 20), [(2000, np.inf)])),
    _case("edges_only", "energy only at the ends of frame 1's window: lag sums that wrap show", 2560, _edges_only),
]
BY_NAME = {c.name: c for c in CASES}

# name -> (stage whose check must fail, cases).  Every listed case is run; the mutant must fail the stage in at least one.
MUTANTS = {
    "symmetric_hann": ("r", ["music40", "L2560"]),
    "offset_511": ("r", ["music40", "L2560"]),
    "no_loading": ("a", ["music40", "sine"]),
    "lags_wrap": ("r", ["edges_only"]),
    "reflection_sign": ("a", ["music40"]),
    "neighbour_a": ("e", ["music40", "L4133"]),
    "upper_median": ("sigma", ["live1000", "L2560"]),
    "c_0675": ("sigma", ["music40"]),
    "ge_for_gt": ("flags", ["at_threshold"]),
    "dilate_short": ("mask", ["edges", "merge"]),
    "dilate_in_frame": ("mask", ["edges"]),
}


# ------------------------------------------------------------------------------------------------------------------ shared pieces
def segments(y, off=LEAD):
    """(F, 2048): row j holds y[jN - off + i], zero outside [0, L)"""
    L = y.shape[0]
    F = frames(L)
    pad = np.zeros(off + F * N + W, y.dtype)
    pad[off:off + L] = y
    return np.stack([pad[j * N:j * N + W] for j in range(F)])


def levinson(r, dtype, loading=LOADING, fma=None, sign=1.0):
    """r (17,) -> a (16,) in `dtype`; fma(a, b, c) given = the kernel's fused order, else plain float64 arithmetic"""
    a = np.zeros(P + 1, dtype)
    if not (np.isfinite(r[0]) and r[0] > 0):
        return a[1:]
    one = dtype(1.0)
    E = dtype(r[0]) * dtype(f32(1.0 + loading) if dtype is f32 else 1.0 + loading)
    for m in range(1, P + 1):
        acc = dtype(r[m])
        for i in range(1, m):
            acc = fma(-a[i], dtype(r[m - i]), acc) if fma else acc - a[i] * r[m - i]
        k = dtype(acc / E)
        an = a.copy()
        for i in range(1, m):
            an[i] = fma(dtype(-sign) * k, a[m - i], a[i]) if fma else a[i] - sign * k * a[m - i]
        an[m] = k
        a = an
        E = (fma(-k, k, one) if fma else one - k * k) * E
    return a[1:]


def residual(y, a, dtype, fma=None, shift=0):
    """e (L,) in `dtype` from y (L,) and a (F, 16); shift: the frame whose a is used is j + shift (clamped) -- a mutant"""
    L = y.shape[0]
    F = frames(L)
    pad = np.concatenate([np.zeros(P, dtype), y.astype(dtype)])
    fr = np.clip(np.arange(L) // N + shift, 0, F - 1)
    acc = np.zeros(L, dtype)
    for i in range(1, P + 1):
        ai, yi = a[fr, i - 1].astype(dtype), pad[P - i:P - i + L]
        acc = fma(ai, yi, acc) if fma else acc + ai * yi
    return (y.astype(dtype) - acc).astype(dtype)


def _rank_select(vals, c, upper=False):
    """the element of rank ceil(c / 2) (1-based; `upper`: floor(c / 2) + 1) of non-negative `vals`, NaNs last"""
    s = np.sort(vals)                                            # numpy sorts NaN last
    return s[(c // 2) if upper else ((c + 1) // 2 - 1)]


def sigma_from_e(e32, L, upper=False, c_mad=C_MAD):
    """bit for bit: per frame the |e| of rank ceil(c / 2) by the uint32 pattern, divided once by 0.6745f"""
    out = np.zeros(frames(L), f32)
    for j in range(frames(L)):
        c = live(L, j)
        keys = np.sort(np.abs(e32[j * N:j * N + c]).view(np.uint32))
        with np.errstate(invalid="ignore"):
            out[j] = keys[(c // 2) if upper else ((c + 1) // 2 - 1):][:1].view(f32)[0] / c_mad
    return out


def flags_from(e, sigma, L, K, floor, dtype=f32, ge=False):
    """flags (L,) uint8 from e and the per-frame sigma: |e| > K * (sigma > floor ? sigma : floor), strict, NaN never"""
    s = np.repeat(sigma.astype(dtype), N)[:L]
    with np.errstate(invalid="ignore"):
        thr = dtype(K) * np.where(s > dtype(floor), s, dtype(floor)).astype(dtype)
        a = np.abs(e.astype(dtype))
        return ((a >= thr) if ge else (a > thr)).astype(np.uint8), thr


def mask_from(flags, guard, short=False, in_frame=False):
    """mask (L,) fp32 and the count of zeros; `short`: one sample less on the right; `in_frame`: the dilation stops at frame boundaries"""
    L = flags.shape[0]
    m = np.ones(L, f32)
    for q in np.flatnonzero(flags):
        lo, hi = max(0, q - guard), min(L - 1, q + guard - (1 if short else 0))
        if in_frame:
            lo, hi = max(lo, (q // N) * N), min(hi, (q // N) * N + N - 1)
        m[lo:hi + 1] = 0.0
    return m, int((m == 0).sum())


def ref_mask_rows(x, m, L, Ly):
    out = np.zeros((x.shape[0], Ly), f32)
    out[:, :L] = x[:, :L].astype(f32) * m
    return out


def ref_blend(x, y, m, L, fade):
    """(B, L): y where no zero of m lies within `fade`, x on the zeros, else fl(fl(w y) + fl(fl(1 - w) x)), w = fl(d / (fade + 1))"""
    m = np.broadcast_to(m, (x.shape[0], L))
    out = y[:, :L].astype(f32).copy()
    for b in range(x.shape[0]):
        zeros = np.flatnonzero(m[b] == 0)
        if zeros.size == 0:
            continue
        n = np.arange(L)
        idx = np.searchsorted(zeros, n)
        left = np.where(idx > 0, n - zeros[np.clip(idx - 1, 0, zeros.size - 1)], 10 ** 9)
        right = np.where(idx < zeros.size, zeros[np.clip(idx, 0, zeros.size - 1)] - n, 10 ** 9)
        d = np.minimum(left, right)
        w = (d.astype(f32) / f32(fade + 1)).astype(f32)
        mix = (w * y[b, :L].astype(f32)).astype(f32) + ((f32(1.0) - w).astype(f32) * x[b, :L].astype(f32)).astype(f32)
        out[b] = np.where(d == 0, x[b, :L], np.where(d <= fade, mix.astype(f32), y[b, :L]))
    return out


# ------------------------------------------------------------------------------------------------------------------ model
def hann64():
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(W) / W)


def model_r(y):
    """-> (r (F, 17) float64, sum_i |s_i s_{i+k}| (F, 17)) from fp32 y taken as float64"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = segments(y.astype(f64)) * hann64()
        r = np.stack([(s[:, :W - k] * s[:, k:]).sum(axis=1) for k in range(P + 1)], axis=1)
        mag = np.stack([np.abs(s[:, :W - k] * s[:, k:]).sum(axis=1) for k in range(P + 1)], axis=1)
    return r, mag


def model(y, K=K_DEF, floor=FLOOR_DEF, guard=GUARD_DEF):
    """the whole detector in float64 -> namespace(r, a, e, sigma, ratio, flags, mask, masked, undecided)"""
    L = y.shape[0]
    r, _ = model_r(y)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a = np.stack([levinson(r[j], f64) for j in range(frames(L))])
        e = residual(y, a, f64)
        sigma = np.array([_rank_select(np.abs(e[j * N:j * N + live(L, j)]), live(L, j)) for j in range(frames(L))]) / f64(C_MAD)
        flags, thr = flags_from(e, sigma, L, f64(f32(K)), f64(f32(floor)), dtype=f64)
        ratio = np.abs(e) / thr
        undecided = (ratio >= 1 - TAU) & (ratio <= 1 + TAU)
    mask, masked = mask_from(flags, guard)
    return SimpleNamespace(r=r, a=a, e=e, sigma=sigma, ratio=ratio, flags=flags, mask=mask, masked=masked, undecided=undecided)


# ------------------------------------------------------------------------------------------------------------------ emulation
def fma32(a, b, c):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def emulate(y, K=K_DEF, floor=FLOOR_DEF, guard=GUARD_DEF, mutant=None):
    """fp32 in the kernel's order -> namespace(r, a, e, sigma, flags, mask, masked)"""
    L = y.shape[0]
    F = frames(L)
    i = np.arange(W)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if mutant == "symmetric_hann":
            h = (0.5 - 0.5 * np.cos(2 * np.pi * i / (W - 1))).astype(f32)
        else:
            w = np.sin(np.pi * (i / W)).astype(f32)
            h = (w * w).astype(f32)
        seg = segments(y.astype(f32), off=LEAD - 1 if mutant == "offset_511" else LEAD)
        s = (h[None] * seg).astype(f32)
        r = np.zeros((F, P + 1), f32)
        for k in range(P + 1):
            p = np.zeros((F, 256), f32)
            for q in range(W // 256):
                t = np.arange(256) + 256 * q
                if mutant == "lags_wrap":
                    p = fma32(s[:, t], s[:, (t + k) % W], p)
                else:
                    ok = t + k < W
                    p[:, ok] = fma32(s[:, t[ok]], s[:, t[ok] + k], p[:, ok])
            p = p.reshape(F, 4, 64)
            for o in (32, 16, 8, 4, 2, 1):
                p = (p[:, :, :o] + p[:, :, o:2 * o]).astype(f32)
            r[:, k] = ((p[:, 0, 0] + p[:, 1, 0]).astype(f32) + (p[:, 2, 0] + p[:, 3, 0]).astype(f32)).astype(f32)
        a = np.stack([levinson(r[j], f32, loading=0.0 if mutant == "no_loading" else LOADING, fma=fma32,
                               sign=-1.0 if mutant == "reflection_sign" else 1.0) for j in range(F)])
        e = residual(y.astype(f32), a, f32, fma=fma32, shift=1 if mutant == "neighbour_a" else 0)
        sigma = sigma_from_e(e, L, upper=mutant == "upper_median", c_mad=f32(0.675) if mutant == "c_0675" else C_MAD)
        flags, _ = flags_from(e, sigma, L, K, floor, ge=mutant == "ge_for_gt")
    mask, masked = mask_from(flags, guard, short=mutant == "dilate_short", in_frame=mutant == "dilate_in_frame")
    return SimpleNamespace(r=r, a=a, e=e, sigma=sigma, flags=flags, mask=mask, masked=masked)


# ------------------------------------------------------------------------------------------------------------------ checks
def bound_r(y):
    _, mag = model_r(y)
    return gamma(32) * mag + 4096 * TINY


def bound_e(y, a):
    L = y.shape[0]
    pad = np.concatenate([np.zeros(P), np.abs(y.astype(f64))])
    fr = np.arange(L) // N
    with np.errstate(invalid="ignore", over="ignore"):
        tot = np.abs(y.astype(f64))
        for i in range(1, P + 1):
            tot = tot + np.abs(a[fr, i - 1].astype(f64)) * pad[P - i:P - i + L]
    return gamma(P + 2) * tot + TINY


def ratio(got, want, bnd):
    """largest |got - want| / bound; where the model is not finite the result must be non-finite too (and is left out); a zero bound needs
    an exact match"""
    got, want, bnd = np.asarray(got, f64), np.asarray(want, f64), np.asarray(bnd, f64)
    skip = ~np.isfinite(want)
    if np.any(np.isfinite(got[skip])):
        return math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - want)[~skip]
        if not np.all(np.isfinite(err)):
            return math.inf
        rr = np.where(err == 0, 0.0, err / bnd[~skip])
    return float(np.max(rr)) if rr.size else 0.0


def a_reference(r32):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return np.stack([levinson(r32[j].astype(f64), f64) for j in range(r32.shape[0])])


def a_error(out):
    """largest |a32 - a64| of `out`, a64 the float64 Levinson-Durbin on out's own fp32 r (NaN -> inf)"""
    err = np.abs(out.a.astype(f64) - a_reference(out.r))
    return float(np.max(err)) if np.all(np.isfinite(err)) else math.inf


_tol_cache = {}


def a_tolerance(case):
    """A_FACTOR times the emulation's own largest |a32 - a64| on this case"""
    if case.name not in _tol_cache:
        _tol_cache[case.name] = A_FACTOR * a_error(emulate(case.make(), case.K, case.floor, case.guard))
    return _tol_cache[case.name]


def check_stages(case, y, out):
    """teacher-forced stage checks of `out` (the kernel's or the emulation's r, a, e, sigma, flags, mask, masked for the clip y) ->
    dict stage -> figure; a stage passes when its figure is <= 1 (bounded stages: the largest error / bound; exact stages: 0 or inf)"""
    L = y.shape[0]
    res = {}
    r64, _ = model_r(y)
    res["r"] = ratio(out.r, r64, bound_r(y))
    tol, err = a_tolerance(case), a_error(out)
    res["a"] = 0.0 if err == 0 else (err / tol if tol > 0 else math.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        res["e"] = ratio(out.e, residual(y, out.a.astype(f64), f64), bound_e(y, out.a))
    exact = lambda got, want: 0.0 if np.array_equal(np.asarray(got).view(np.uint32) if np.asarray(got).dtype == f32 else np.asarray(got),
                                                    np.asarray(want).view(np.uint32) if np.asarray(want).dtype == f32 else np.asarray(want)) else math.inf
    res["sigma"] = exact(out.sigma.astype(f32), sigma_from_e(out.e.astype(f32), L))
    res["flags"] = exact(out.flags.astype(np.uint8), flags_from(out.e.astype(f32), out.sigma.astype(f32), L, case.K, case.floor)[0])
    m, cnt = mask_from(out.flags, case.guard)
    res["mask"] = 0.0 if (np.array_equal(np.asarray(out.mask, f32), m) and int(out.masked) == cnt) else math.inf
    return res


def end_to_end(case, y, mask):
    """-> (bad, undecided share): bad = samples where `mask` differs from the model's and no undecided sample lies within `guard`"""
    mo = model(y, case.K, case.floor, case.guard)
    near = mask_from(mo.undecided.astype(np.uint8), case.guard)[0] == 0
    bad = int(((np.asarray(mask, f32) != mo.mask) & ~near).sum())
    return bad, float(mo.undecided.mean())
