"""Shared by tests/test_warp_bound_host.py (CPU) and tests/test_gpu_time_warp.py (GPU): a float64 model of the time-warp operator and of its
transpose (csrc/warp.hip), an element-wise bound, an fp32 emulation in the kernels' documented order, mutants and
the case table.  Written the way tests/drc_cases.py is; no GPU dependency.

MODEL (float64, from the definition; `model`, `model_bwd`, `model_bwd_scatter`).  Per clip, x zero outside [0, L), H = ceil(L / 64), the
curve H + 1 fp32 knots d[0 .. H] in samples (taken as float64 values of fp32 numbers):

    n = 64 j + r     delta(n) = d[j] + (r / 64) (d[j+1] - d[j])     i(n) = n + floor(delta)     f(n) = delta - floor(delta) in [0, 1)
    w[-1] = -0.5 f^3 + f^2 - 0.5 f    w[0] = 1.5 f^3 - 2.5 f^2 + 1    w[1] = -1.5 f^3 + 2 f^2 + 0.5 f    w[2] = 0.5 f^3 - 0.5 f^2
    y[n]  = sum over k = -1 .. 2 with 0 <= i + k < L of w[k] x[i + k]
    dx[m] = sum over n with i(n) in [m - 2, m + 1] of w[m - i(n)](f(n)) dy[n]        (gather form, ascending n; zero on [L, full))

  `model_bwd` is the gather form the kernel uses: i(n) is non-decreasing under the curve's contract, so the contributors of m are found by
  a sorted search and at most GATHER_CAP = 8 of them are visited (six exist at most).  `model_bwd_scatter` adds w[k] dy[n] into dx[i + k].

BOUND, from the number formats alone (u = 2^-24, gamma(n) = n u / (1 - n u); `bound`, `bound_bwd`), evaluated at the model's (i, f).  Write
the interpolant as y[n] = sum_t h(t - n - delta) x[t] with the Catmull-Rom basis function h (support (-2, 2), C^1, |h''| <= 5 piecewise):
the weights are w[k](f) = h(k - f), and a floor() that the kernel and the model decide differently is the SAME h at nearly the same point.
    delta     the kernel's delta = fmaf(r / 64, d[j+1] - d[j], d[j]) has one rounding in the difference and one in the fmaf, the fraction
              f = delta - floorf(delta) one more (inexact only for a small negative delta, where it matters: |w'| is not small next to |w|
              there):  |delta32 - delta| + |f's rounding| <= eps = 2 u (|d[j]| + |d[j+1]| + |delta| + 1)                    (a factor 2 of slack)
    h         first order |sum_k w'[k](f) x_k| eps (the signed sum: it cancels for smooth x, and that is what makes the bound tight);
              second order (1/2) max |h''| eps^2 = 2.5 eps^2 per tap, taken as 3 eps^2 over the SIX taps i - 2 .. i + 3 that h can reach
              from a point within eps of the model's (the four of the model and one more on either side)
    weights   rounding of the Horner forms at an exact f, propagated operation by operation with each intermediate's range on [0, 1]:
              |w32[k] - w[k]| <= E[k] u, E = (1.6, 6, 4.2, 1.1) for k = -1 .. 2.  Where f lies within eps of 0 or 1 the kernel may hold
              the neighbouring cell's weights: there 6 u on all six taps
    sum       acc = fmaf(w, x, acc) per tap, four roundings: gamma(5) sum_k |w[k] x_k| (one of slack for the computed weights)
    floor     2^-126, the most a rounding can lose below the normal range, flushed or not
  |y[n] - model| <= sum_k E[k] u |x_k| + gamma(5) sum_k |w[k] x_k| + |sum_k w'[k] x_k| eps + 3 eps^2 sum_{six} |x_t| + 2^-126.
  The issue's starting point had 8 u sum |x_k| for the first two terms; this one is derived term by term and is smaller for most f.
  Transpose: the same terms per contributing n with |dy[n]| in place of |x_k| and eps of that n -- E[c] u |dy_n|, |w'[c](f_n)| |dy_n| eps_n
  (no cancellation to use: every n has its own f) -- the second-order term over the n with i(n) in [m - 3, m + 2] (c = -2 and c = 3 carry
  weight 0 in the model and at most 3 eps^2 in the kernel), and the chain of at most 8 fmaf: gamma(9) sum_n |w dy_n|.
  A relative weight term (eps |w|) or an eps without the + 1 does NOT hold for small negative delta: case `tiny_negative` keeps that honest.

EMULATION (`emulate`, `emulate_bwd`): numpy float32 in the kernels' order; fmaf(a, b, c) is evaluated in float64 (the product of two fp32
numbers is exact there) and rounded to fp32.  It validates the bound on the CPU; it is not a second oracle.

MUTANTS: `MUTANTS` maps a name to (stage, case names); each must leave the bound in at least one element of one listed case.

CASES: see `CASES`; every case carries `why`.  Inputs are seeded standard-normal x and dy."""
import math
import zlib
from types import SimpleNamespace

import numpy as np

from tests import spectral_cases as S

U, gamma, ratio = S.U, S.gamma, S.ratio
f32, f64 = np.float32, np.float64
R = 64
MAX_DELAY, MAX_STEP = 4096.0, 16.0
GATHER_CAP = 8
TINY = 2.0 ** -126
E_W = (1.6, 6.0, 4.2, 1.1)          # rounding of the four Horner forms, in units of u
FS = 16000


def blocks(L):
    return -(-L // R)


def knots(L):
    return blocks(L) + 1


# ------------------------------------------------------------------------------------------------------------------ cases and inputs
def _case(name, why, L, curve="walk", step=4.0, B=3, full=None, stride=None, off=0, shared=False, signal="randn"):
    full = full or L
    return SimpleNamespace(name=name, why=why, L=L, H=blocks(L), K=knots(L), curve=curve, step=step, B=B, full=full, stride=stride or L, off=off,
                           shared=shared, signal=signal)


FWD_SPAN, BWD_SPAN = 1024, 256      # samples per workgroup of warp_fwd (256 threads x 4 outputs) and warp_bwd (256 threads x 1 input)

CASES = [
    _case("L1", "a single sample: two knots, three of four taps outside", 1, step=0.3),
    _case("L5", "two knots, shorter than the four taps reach", 5, step=1.5),
    _case("L63", "one block, one sample short", 63),
    _case("L64", "exactly one block: two knots", 64),
    _case("L65", "one block and one sample: three knots", 65, full=70),
    _case("L255", "one below warp_bwd's workgroup span", BWD_SPAN - 1),
    _case("L256", "warp_bwd's workgroup span", BWD_SPAN),
    _case("L257", "one above warp_bwd's workgroup span", BWD_SPAN + 1, full=BWD_SPAN + 2),
    _case("L1023", "one below warp_fwd's workgroup span", FWD_SPAN - 1),
    _case("L1024", "warp_fwd's workgroup span", FWD_SPAN),
    _case("L1025", "one above warp_fwd's workgroup span", FWD_SPAN + 1),
    _case("L1000", "a partial last block of 40 samples; full > L", 1000, full=1003),
    _case("L6400_zigzag", "+-16 per block, alternating: extreme slopes change every block, six contributors per input", 6400, "zigzag"),
    _case("L6400_faster", "16 more per block until the clamp at +4096: speed 1.25, then 1", 6400, "faster"),
    _case("L6400_slower", "16 less per block until the clamp at -4096: speed 0.75, then 1", 6400, "slower", full=6432),
    _case("L1000_const300", "a constant +300, -300, +300.25: most taps of the ends lie outside the clip", 1000, "const300"),
    _case("L1000_integers", "knots that are exact integers, some blocks flat: floorf ties, f = 0", 1000, "integers"),
    _case("L1000_tiny_negative", "knots of -1e-4, -1e-8 and mixed tiny values: f rounds towards, and to, 1.0", 1000, "tiny_negative"),
    _case("L20037_stride", "odd length, an unaligned row offset, row stride above L, full > L; y rows alternate in alignment", 20037, full=20100,
          stride=20101, off=1, step=16.0),
    _case("L70000", "H = 1094, a curve per clip, steps up to 16", 70000, step=16.0),
    _case("L70000_shared", "the same length with one shared curve (delay_stride 0)", 70000, step=0.3, shared=True),
    _case("L20000_wow", "wow_curve: 0.5 Hz / 1 % wow plus 9 Hz / 0.2 % flutter, shared", 20000, "wow", shared=True),
    _case("L6400_silence", "all zeros in, all zeros out", 6400, signal="silence"),
]
CASE = {c.name: c for c in CASES}


def _rng(name, tag):
    return np.random.default_rng(zlib.crc32(f"warp/{name}/{tag}".encode()))


def random_walk(rng, K, step, start):
    """K knots: a walk with uniform steps in [-step, step], reflected into +-MAX_DELAY, rounded to fp32 with the step limit kept"""
    d = np.empty(K)
    d[0] = start
    for j in range(1, K):
        s = rng.uniform(-step, step)
        d[j] = d[j - 1] + (s if abs(d[j - 1] + s) <= MAX_DELAY else -s)
    d = d.astype(f32)
    for j in range(1, K):                                       # rounding may push a step of exactly 16 over: pull it back
        if abs(f64(d[j]) - f64(d[j - 1])) > MAX_STEP:
            d[j] = np.nextafter(d[j], d[j - 1])
    return d


def curve_for(c):
    """the case's knots, (K,) when shared, (B, K) otherwise; fp32, inside the contract"""
    rng = _rng(c.name, "curve")
    K, j = c.K, np.arange(c.K)
    if c.curve == "walk":
        lim = min(MAX_DELAY, c.L / 4.0)                         # short clips keep their taps inside; clip 0 of a long one may start anywhere
        rows = [random_walk(rng, K, c.step, start=rng.uniform(-lim, lim) if b == 0 else rng.uniform(-min(lim, 40.0), min(lim, 40.0)))
                for b in range(c.B)]
    elif c.curve == "zigzag":
        rows = [np.where(j % 2 == 0, a, -a).astype(f32) for a in (8.0, -8.0, 7.96875)]
    elif c.curve == "faster":
        rows = [np.minimum(s + 16.0 * j, MAX_DELAY).astype(f32) for s in (3000.0, 3500.5, -100.0)]
    elif c.curve == "slower":
        rows = [np.maximum(s - 16.0 * j, -MAX_DELAY).astype(f32) for s in (-3000.0, -3500.5, 100.0)]
    elif c.curve == "const300":
        rows = [np.full(K, v, f32) for v in (300.0, -300.0, 300.25)]
    elif c.curve == "integers":
        rows = [np.cumsum(rng.integers(-3, 4, K) * (rng.random(K) < 0.6)).astype(f32) + f32(o) for o in (0.0, -7.0, 12.0)]
    elif c.curve == "tiny_negative":
        rows = [np.full(K, -1e-4, f32), np.full(K, -1e-8, f32), (rng.choice([-1.0, 1.0], K) * 10.0 ** rng.uniform(-9, -3, K)).astype(f32)]
    elif c.curve == "wow":
        from diffmusic_amd.inverse_problem.dsp import wow_curve
        rows = [wow_curve(c.L, FS, ((0.5, 1.0, 0.0), (9.0, 0.2, 0.0)))]
    else:
        raise KeyError(c.curve)
    d = np.stack(rows[:c.B]).astype(f32)
    return d[0].copy() if c.shared else d


_INPUTS = {}


def inputs(c):
    """everything a case feeds the kernels, fp32 numpy, identical on the host and the GPU side; cached and never modified"""
    if c.name not in _INPUTS:
        store = _rng(c.name, "x").standard_normal((c.B, c.stride)).astype(f32)
        if c.signal == "silence":
            store[:] = 0
        dy = _rng(c.name, "dy").standard_normal((c.B, c.L)).astype(f32)
        d = curve_for(c)
        assert d.dtype == f32 and d.shape == ((c.K,) if c.shared else (c.B, c.K)) and in_contract(d), c.name
        _INPUTS[c.name] = SimpleNamespace(store=store, x=store[:, :c.L], dy=dy, delay=d)
    return _INPUTS[c.name]


def in_contract(d):
    d = np.asarray(d, f64)
    return bool(np.isfinite(d).all() and np.abs(d).max() <= MAX_DELAY and np.abs(np.diff(d, axis=-1)).max() <= MAX_STEP)


def rows_of(delay, B, mut=None):
    """(K,) or (B, K) -> (B, K) float64"""
    d = np.asarray(delay, f64)
    d = np.broadcast_to(d, (B, d.shape[-1])) if d.ndim == 1 else d
    return np.broadcast_to(d[:1], d.shape) if mut == "curve_row_0" else d


# ------------------------------------------------------------------------------------------------------------------ float64 model
def weights(f, mut=None):
    """(4, ...) the weights of the taps k = -1 .. 2, and their derivatives in f"""
    w = np.stack([((-0.5 * f + 1.0) * f - 0.5) * f, (1.5 * f - 2.5) * f * f + 1.0, ((-1.5 * f + 2.0) * f + 0.5) * f, (0.5 * f - 0.5) * f * f])
    dw = np.stack([(-1.5 * f + 2.0) * f - 0.5, (4.5 * f - 5.0) * f, (-4.5 * f + 4.0) * f + 0.5, (1.5 * f - 1.0) * f])
    if mut == "linear":
        w = np.stack([0.0 * f, 1.0 - f, f, 0.0 * f])
    if mut == "outer_weights_swapped":
        w = w[[3, 1, 2, 0]]
    return w, dw


def positions(d, L, mut=None):
    """one clip's knots (K,) float64 -> (d0, d1, delta, i, f) over n = 0 .. L - 1"""
    n = np.arange(L)
    j, r = n // R, n % R
    d0, d1 = d[j], d[j + 1]
    delta = d0 + ((r + (1 if mut == "knot_weight_r_plus_1" else 0)) / R) * (d1 - d0)
    fl = np.trunc(delta) if mut == "truncation" else np.floor(delta)
    return d0, d1, delta, n + fl.astype(np.int64), delta - fl


def model(x, delay, L, mut=None):
    """float64 forward: x (B, >= L), delay (K,) or (B, K) -> namespace; r.y (B, L), r.i, r.f, r.eps (B, L)"""
    x = np.asarray(x, f64)[:, :L]
    B = x.shape[0]
    D = rows_of(delay, B, mut)
    r = SimpleNamespace(y=np.zeros((B, L)), i=np.zeros((B, L), np.int64), f=np.zeros((B, L)), eps=np.zeros((B, L)), first=np.zeros((B, L)),
                        absw=np.zeros((B, L)), round_w=np.zeros((B, L)), six=np.zeros((B, L)))
    for b in range(B):
        d0, d1, delta, i, f = positions(D[b], L, mut)
        w, dw = weights(f, mut)
        shift = 1 if mut == "taps_one_on" else 0
        xp = np.concatenate([np.zeros(3), x[b], np.zeros(4)])           # x[t] at xp[t + 3], zero outside
        for k in range(-1, 3):
            t = i + k + shift
            if mut == "taps_clamped":
                xt = x[b][np.clip(t, 0, L - 1)]
            else:
                xt = np.where((t >= 0) & (t < L), xp[np.clip(t + 3, 0, L + 6)], 0.0)
            r.y[b] += w[k + 1] * xt
            r.first[b] += dw[k + 1] * xt
            r.absw[b] += np.abs(w[k + 1] * xt)
            r.round_w[b] += E_W[k + 1] * np.abs(xt)
        for k in range(-2, 4):
            t = i + k
            r.six[b] += np.where((t >= 0) & (t < L), np.abs(xp[np.clip(t + 3, 0, L + 6)]), 0.0)
        r.i[b], r.f[b] = i, f
        r.eps[b] = 2.0 * U * (np.abs(d0) + np.abs(d1) + np.abs(delta) + 1.0)
    return r


def _gather(i, L, lo_off, hi_off, cap):
    """one clip: visit, for every m, the n ascending from the first with i(n) >= m - lo_off while i(n) <= m + hi_off, at most `cap` of them
    -> lists of (n, c = m - i(n), valid) per visit"""
    m = np.arange(L)
    lo = np.searchsorted(i, m - lo_off, side="left")
    for q in range(cap):
        n = lo + q
        nc = np.minimum(n, L - 1)
        valid = (n < L) & (i[nc] <= m + hi_off)
        yield nc, m - i[nc], valid


def model_bwd(dy, delay, L, r, mut=None):
    """float64 transpose in gather form, with the (i, f, eps) of the forward model r -> namespace; rb.dx (B, L) and the bound's sums"""
    dy = np.asarray(dy, f64)[:, :L]
    B = dy.shape[0]
    rb = SimpleNamespace(dx=np.zeros((B, L)), count=np.zeros((B, L), np.int64), round_w=np.zeros((B, L)), first=np.zeros((B, L)),
                         absw=np.zeros((B, L)), second=np.zeros((B, L)))
    lo_off = 1 if mut == "range_short_below" else 2
    hi_off = 0 if mut == "range_short_above" else 1
    src = 0 if mut == "curve_row_0" else None
    for b in range(B):
        i, f, eps = (r.i[b], r.f[b], r.eps[b]) if src is None else (r.i[src], r.f[src], r.eps[src])
        assert np.all(np.diff(i) >= 0), "i(n) must be non-decreasing for the gather form"
        w, dw = weights(f)
        EW = np.asarray(E_W)
        for n, c, valid in _gather(i, L, lo_off, hi_off, GATHER_CAP):
            k = np.clip(c + 1, 0, 3)
            wk, dwk, g = w[k, n], dw[k, n], dy[b][n]
            rb.dx[b] += np.where(valid, wk * g, 0.0)
            rb.count[b] += valid
            rb.round_w[b] += np.where(valid, EW[k] * np.abs(g), 0.0)
            rb.first[b] += np.where(valid, np.abs(dwk * g) * eps[n], 0.0)
            rb.absw[b] += np.where(valid, np.abs(wk * g), 0.0)
        seen = np.zeros(L, np.int64)
        for n, c, valid in _gather(i, L, 3, 2, GATHER_CAP + 4):           # the six offsets c = -2 .. 3 h can reach
            rb.second[b] += np.where(valid, np.abs(dy[b][n]) * eps[n] ** 2, 0.0)
            seen += valid
        lo = np.searchsorted(i, np.arange(L) - 3, side="left")
        assert np.array_equal(seen, np.searchsorted(i, np.arange(L) + 2, side="right") - lo), "the wide gather visited every n it should"
    return rb


def model_bwd_scatter(dy, L, r):
    """the same transpose as a scatter: w[k](f(n)) dy[n] added into dx[i(n) + k]"""
    dy = np.asarray(dy, f64)[:, :L]
    dx = np.zeros(dy.shape)
    for b in range(dy.shape[0]):
        w, _ = weights(r.f[b])
        for k in range(-1, 3):
            t = r.i[b] + k
            ok = (t >= 0) & (t < L)
            np.add.at(dx[b], t[ok], (w[k + 1] * dy[b])[ok])
    return dx


# ------------------------------------------------------------------------------------------------------------------ the bound
def near_cell_edge(r):
    return (r.f <= r.eps) | (r.f >= 1.0 - r.eps)


def bound(r):
    """element-wise bound (B, L) on |kernel - model| of y for the model run r"""
    rounding = np.where(near_cell_edge(r), 6.0 * r.six, r.round_w) * U
    return rounding + gamma(5) * r.absw + np.abs(r.first) * r.eps + 3.0 * r.eps ** 2 * r.six + TINY


def bound_bwd(r, rb, dy):
    """element-wise bound (B, L) on |kernel - model| of dx for the model transpose rb.  A contributor near a cell edge may carry the
    neighbouring cell's weight in the kernel: 6 u |dy[n]| for every n in the wide set covers it (`wide_abs`)"""
    dy = np.abs(np.asarray(dy, f64))
    B, L = dy.shape
    wide = np.zeros((B, L))
    for b in range(B):
        for n, c, valid in _gather(r.i[b], L, 3, 2, GATHER_CAP + 4):
            edge = (r.f[b][n] <= r.eps[b][n]) | (r.f[b][n] >= 1.0 - r.eps[b][n])
            wide[b] += np.where(valid & edge, 6.0 * dy[b][n], 0.0)
    return (rb.round_w + wide) * U + gamma(9) * rb.absw + rb.first + 3.0 * rb.second + TINY


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation
def fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def weights32(f):
    """the kernel's Horner forms, k = -1 .. 2"""
    f = np.asarray(f, f32)
    ff = f * f
    return [f * fma(fma(f32(-0.5), f, f32(1)), f, f32(-0.5)), fma(fma(f32(1.5), f, f32(-2.5)), ff, f32(1)),
            f * fma(fma(f32(-1.5), f, f32(2)), f, f32(0.5)), ff * fma(f32(0.5), f, f32(-0.5))]


def positions32(d, L):
    """one clip's knots (K,) fp32 -> (i, f) as the kernel computes them"""
    d = np.asarray(d, f32)
    n = np.arange(L)
    j, r = n // R, n % R
    delta = fma((r / R).astype(f32), d[j + 1] - d[j], d[j])
    fl = np.floor(delta)
    f = delta - fl
    assert delta.dtype == f32 and f.dtype == f32
    return n + fl.astype(np.int64), f


def emulate(x, delay, L):
    """fp32 emulation of warp_fwd -> y (B, L)"""
    x = np.asarray(x, f32)[:, :L]
    B = x.shape[0]
    D = rows_of(delay, B).astype(f32)
    y = np.zeros((B, L), f32)
    for b in range(B):
        i, f = positions32(D[b], L)
        w = weights32(f)
        acc = np.zeros(L, f32)
        for k in range(-1, 3):
            t = i + k
            ok = (t >= 0) & (t < L)
            acc = np.where(ok, fma(w[k + 1], x[b][np.clip(t, 0, L - 1)], acc), acc)
        y[b] = acc
    return y


def emulate_bwd(dy, delay, L):
    """fp32 emulation of warp_bwd -> dx (B, L): the search of the first n with i(n) >= m - 2, then at most GATHER_CAP terms ascending"""
    dy = np.asarray(dy, f32)[:, :L]
    B = dy.shape[0]
    D = rows_of(delay, B).astype(f32)
    dx = np.zeros((B, L), f32)
    m = np.arange(L)
    for b in range(B):
        i, f = positions32(D[b], L)
        assert np.all(np.diff(i) >= 0)
        w = np.stack(weights32(f))
        lo = np.searchsorted(i, m - 2, side="left")
        acc = np.zeros(L, f32)
        for q in range(GATHER_CAP):
            n = np.minimum(lo + q, L - 1)
            c = m - i[n]
            ok = (lo + q < L) & (c >= -1) & (c <= 2)
            acc = np.where(ok, fma(w[np.clip(c + 1, 0, 3), n], dy[b][n], acc), acc)
        dx[b] = acc
    return dx


# ------------------------------------------------------------------------------------------------------------------ mutants
# name -> (stage: "fwd" judged on y, "bwd" judged on dx; case names).  Every listed case is run; the mutant must leave the bound in at
# least one.
MUTANTS = {
    "taps_one_on": ("fwd", ["L1000", "L65"]),                               # taps i .. i + 3
    "truncation": ("fwd", ["L6400_slower", "L1000_const300"]),              # (int) delta in place of floorf: wrong for negative delta
    "knot_weight_r_plus_1": ("fwd", ["L6400_zigzag", "L1000"]),             # delta from (r + 1) / 64
    "outer_weights_swapped": ("fwd", ["L1000", "L64"]),                     # w[-1] and w[2] swapped
    "linear": ("fwd", ["L1000", "L20000_wow"]),                             # linear interpolation
    "taps_clamped": ("fwd", ["L1000_const300", "L5"]),                      # out-of-range taps read the edge sample instead of nothing
    "range_short_below": ("bwd", ["L1000", "L6400_zigzag"]),                # contributors with i(n) = m - 2 dropped
    "range_short_above": ("bwd", ["L1000", "L6400_zigzag"]),                # contributors with i(n) = m + 1 dropped
    "curve_row_0": ("fwd", ["L1000", "L70000"]),                            # clip b reading curve row 0
    "curve_row_0_bwd": ("bwd", ["L1000", "L70000"]),
}


_RUNS = {}


def reference(c):
    """(model forward r, bound of y, model transpose rb, bound of dx) of a case: computed once, shared, never modified"""
    if c.name not in _RUNS:
        i = inputs(c)
        r = model(i.x, i.delay, c.L)
        rb = model_bwd(i.dy, i.delay, c.L, r)
        _RUNS[c.name] = (r, bound(r), rb, bound_bwd(r, rb, i.dy))
    return _RUNS[c.name]


def run_mutant(c, mut, stage):
    """largest |mutated model - model| / bound"""
    i = inputs(c)
    r, qy, rb, qdx = reference(c)
    mut = mut[:-4] if mut.endswith("_bwd") else mut
    if stage == "fwd":
        return ratio(model(i.x, i.delay, c.L, mut).y, r.y, qy)
    return ratio(model_bwd(i.dy, i.delay, c.L, r, mut).dx, rb.dx, qdx)
