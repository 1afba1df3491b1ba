"""Shared by tests/test_tf_gain_bound_host.py (CPU) and tests/test_gpu_tf_gain.py (GPU): a float64 model of the time-frequency gain
(csrc/tf_gain.hip), its element-wise bound, an fp32 emulation in the kernel's documented order, mutants and the case
table.  Written the way tests/spectral_cases.py is; no GPU dependency.

MODEL (float64, from the definition; `model`): n_fft = 1024, hop = 256, periodic Hann w, x taken as zero outside [0, L)
    frames     t = 0 .. T - 1, T = ceil(L / 256) + 3; frame t covers the samples s = (t - 3) 256 + n, n = 0 .. 1023
    analysis   X[k, t] = sum_n w[n] x[s] exp(-2 pi i k n / 1024), k = 0 .. 512
    gain       Y[k, t] = G[k, t] X[k, t], G real, (513, T) for every clip or (B, 513, T)
    synthesis  f_t = irfft(Y[:, t]);  A(x)[s] = (1 / c) sum_{t covers s} w[n] f_t[n], s in [0, L), c = 1.5

BOUND, from the number formats alone (u = 2^-24, gamma(n) = n u / (1 - n u); `bound`), a componentwise absolute-value propagation of the
model; every line is one line of `bound`.  C_IN and C_FFT are those of spectral_cases.py (same FFT code, csrc/fft1024.h).
    frame      x_n = w_n x_s carries C_IN = 3 roundings (window table, product; the third, the noise FMA of the guidance kernels, is unused
               here and kept so that the constant is the same)
    forward    |dX_k| <= (C_FFT + C_IN) u S_t, S_t = sum_n |w_n x_s| (every path from x_n to X_k has modulus one)
    gain       one rounding per component: |dY_k| <= |G_k| (|dX_k| + u (|X_k| + |dX_k|)); the conjugate half is a copy (exact)
    inverse    over the FULL Hermitian spectrum of 1024 bins, modulus of the complex error, of which the real part is kept:
               |d(1024 f_n)| <= sum_k |dY_k| + C_FFT u sum_k (|Y_k| + |dY_k|), the sums over k = 0 .. 1023
    scale      1 / 1024 is a power of two (exact); the window costs two roundings (table, product):
               b(w_n f_n) = w_n b(f_n) + 2 u w_n (|f_n| + b(f_n))
    OLA, 1/c   four terms summed in fp32 (at most four roundings), fp32(2 / 3) and the product (two more):
               b(A_s) = (1 / c) [sum_t b + gamma(6) sum_t (|w f| + b)]
A is linear and has no gates: no ambiguous elements, no cap -- EVERY element must lie within the bound.  The bound holds with or without FMA
contraction (an FMA has fewer roundings).

EMULATION (`emulate`): numpy float32 in the kernel's order -- slabs of SLAB_HOPS output hops; frames h0 .. h1 + 2 of a slab, frame t into
accumulator (t - h0) % 4, the accumulators summed ((a0 + a1) + a2) + a3, times fp32(2 / 3).  It validates the bound on the CPU and carries
the mutants of the slab / frame-range / gain-addressing logic.  It is not a second oracle.

MUTANTS: `MUTANTS` maps a name to (where it lives, case names); each must leave the bound in at least one element of one listed case.

CASES: see `CASES`; every case carries `why`, the branch it is there for."""
import zlib
from types import SimpleNamespace

import numpy as np

from tests import spectral_cases as S

U, C_IN, C_FFT, gamma, ratio = S.U, S.C_IN, S.C_FFT, S.gamma, S.ratio
f32, f64 = np.float32, np.float64
NF, HOP, NB, HALO = 1024, 256, 513, 3
SLAB_HOPS = 8
SLAB = SLAB_HOPS * HOP
C_OLA = 1.5


def frames(L):
    return -(-L // HOP) + HALO


# ------------------------------------------------------------------------------------------------------------------ cases and inputs
def _case(name, why, L, gain, per_clip=False, B=2, full=None, stride=None, out_stride=None, signal="sine"):
    full = full or L
    return SimpleNamespace(name=name, why=why, L=L, T=frames(L), gain=gain, per_clip=per_clip, B=B, full=full, stride=stride or full,
                           out_stride=out_stride or full, signal=signal)


def _cases():
    out = []
    for L, why in ((300, "shorter than a frame (T = 5)"), (1024, "one frame length"), (1025, "one frame length + 1"),
                   (SLAB, "exactly one slab"), (SLAB + 1, "one slab + 1: a second slab of one sample"),
                   (4999, "odd length, three slabs"), (6400, "a multiple of the hop; the step tests' length")):
        out.append(_case(f"L{L}_ones", why + "; identity", L, "ones"))
        out.append(_case(f"L{L}_rand", why + "; random gain in [-1, 2], shared", L, "rand"))
        out.append(_case(f"L{L}_rand_pc", why + "; random gain, one grid per clip", L, "rand", per_clip=True))
    out.append(_case("L6400_stride", "L = 6432 - 32 with row stride 6432; zero tail up to full", 6400, "rand", full=6416, stride=6432, out_stride=6432))
    out.append(_case("L4999_edge", "-0.0f and a large-magnitude sample", 4999, "rand", per_clip=True, signal="edge"))
    for k in (0, 1, 511, 512):
        out.append(_case(f"L2049_bin{k}", f"a single non-zero bin, k = {k}", SLAB + 1, f"bin{k}"))
        out.append(_case(f"L2049_bin{k}_pc", f"a single non-zero bin, k = {k}, per clip", SLAB + 1, f"bin{k}", per_clip=True))
    for L in (300, SLAB + 1):
        out.append(_case(f"L{L}_frame_first", "a single non-zero frame at t = 0", L, "frame_first"))
        out.append(_case(f"L{L}_frame_last", "a single non-zero frame at t = T - 1", L, "frame_last", per_clip=True))
    out.append(_case("L4999_frame_edge", "a single non-zero frame across a slab edge (t = SLAB_HOPS + 1: computed by slab 0 as halo and by slab 1)",
                     4999, "frame_edge"))
    out.append(_case("L4999_frame_edge_pc", "the same, per clip", 4999, "frame_edge", per_clip=True))
    out.append(_case("L6400_zero_frames", "zero frames 6 .. 12: samples [1536, 2560) are exactly zero", 6400, "zero_frames"))
    out.append(_case("L6400_zero_frames_pc", "zero frames 6 .. 12, per clip", 6400, "zero_frames", per_clip=True))
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}


def _rng(name, tag):
    return np.random.default_rng(zlib.crc32(f"tf/{name}/{tag}".encode()))


def _gain(c):
    T, n = c.T, (c.B if c.per_clip else 1)
    rng = _rng(c.name, "gain")
    rand = rng.uniform(-1.0, 2.0, (n, NB, T))
    kind = c.gain
    if kind == "ones":
        g = np.ones((n, NB, T))
    elif kind == "rand":
        g = rand
    elif kind.startswith("bin"):
        g = np.zeros((n, NB, T))
        g[:, int(kind[3:])] = rand[:, int(kind[3:])]
    elif kind.startswith("frame_"):
        t = {"frame_first": 0, "frame_last": T - 1, "frame_edge": SLAB_HOPS + 1}[kind]
        g = np.zeros((n, NB, T))
        g[:, :, t] = rand[:, :, t]
    elif kind == "zero_frames":
        g = rand.copy()
        g[:, :, 6:13] = 0.0
    else:
        raise KeyError(kind)
    g = g.astype(f32)
    return g if c.per_clip else g[0]


_INPUTS = {}


def inputs(c):
    """everything a case feeds the kernel, fp32 numpy, identical on the host and the GPU side; cached and never modified"""
    if c.name in _INPUTS:
        return _INPUTS[c.name]
    store = S._clips("tf/" + c.name, "rows", c.B, c.stride)           # sine plus noise; the last clip pure noise
    if c.signal == "edge":
        store = store.copy()
        store[:, 17] = f32(-0.0)
        store[:, 100:104] = f32(-0.0)
        store[0, 2500] = f32(3.0e4)
        store[1, c.L - 1] = f32(-1.0e3)
    i = SimpleNamespace(store=store, x=store[:, :c.L], gain=_gain(c))
    _INPUTS[c.name] = i
    return i


# ------------------------------------------------------------------------------------------------------------------ float64 model
def window(mut=None):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NF) / (NF - 1 if mut == "hann_symmetric" else NF))


def frame_index(L, T, mut=None):
    """(T, 1024) sample index of position n of frame t (outside [0, L): the zero extension)"""
    return (np.arange(T)[:, None] - (2 if mut == "frame_offset_2" else HALO)) * HOP + np.arange(NF)[None]


def _gain_btk(G, B, mut=None):
    """(513, T) or (B, 513, T) -> (B, T, 513) float64"""
    G = np.asarray(G, f64)
    if G.ndim == 2:
        G = np.broadcast_to(G, (B,) + G.shape)
    elif mut == "gain_of_clip_0":
        G = np.broadcast_to(G[:1], G.shape)
    G = G.transpose(0, 2, 1).copy()
    if mut == "nyquist_from_511":
        G[..., 512] = G[..., 511]
    return G


def model(x, G, L, mut=None):
    """float64 A(x): x (B, >= L), G (513, T) or (B, 513, T) -> namespace with every intermediate; r.y (B, L)"""
    x = np.asarray(x, f64)[:, :L]
    B, T = x.shape[0], frames(L)
    r = SimpleNamespace(T=T)
    r.s = frame_index(L, T, mut)
    inside = (r.s >= 0) & (r.s < L)
    r.win = window(mut)
    r.xw = np.where(inside[None], x[:, np.clip(r.s, 0, L - 1)], 0.0) * r.win
    r.X = np.fft.rfft(r.xw, axis=-1)                               # (B, T, 513)
    r.Y = _gain_btk(G, B, mut) * r.X
    if mut == "frame_last_skipped":
        r.Y[:, T - 1] = 0.0
    if mut == "no_conjugation":                                    # upper half = the lower half itself
        full = np.concatenate([r.Y, r.Y[..., 511:0:-1]], axis=-1)
        r.f = np.fft.ifft(full, axis=-1).real
    else:
        r.f = np.fft.irfft(r.Y, n=NF, axis=-1)
    r.wf = r.f * r.win
    y = np.zeros((B, L))
    for b in range(B):
        np.add.at(y[b], r.s[inside], r.wf[b][inside])
    r.y = y if mut == "no_inv_c" else y / C_OLA
    return r


def bound(x, G, L, r):
    """element-wise bound (B, L) on |kernel - model| for the model run r"""
    B, T = r.xw.shape[0], r.T
    g = np.abs(_gain_btk(G, B))
    S_t = np.abs(r.xw).sum(-1, keepdims=True)
    bX = (C_FFT + C_IN) * U * S_t * np.ones_like(g)
    aX = np.abs(r.X)
    bY = g * (bX + U * (aX + bX))
    aY = np.abs(r.Y)
    herm = np.ones(NB)
    herm[1:512] = 2.0                                             # bins 1 .. 511 appear twice in the full spectrum
    bF = ((bY * herm).sum(-1, keepdims=True) + C_FFT * U * ((aY + bY) * herm).sum(-1, keepdims=True)) / NF
    bwf = r.win * bF + 2 * U * r.win * (np.abs(r.f) + bF)
    inside = (r.s >= 0) & (r.s < L)
    sb, sa = np.zeros((B, L)), np.zeros((B, L))
    for b in range(B):
        np.add.at(sb[b], r.s[inside], bwf[b][inside])
        np.add.at(sa[b], r.s[inside], np.abs(r.wf[b])[inside])
    return (sb + gamma(6) * (sa + sb)) / C_OLA


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation
def emulate(x, G, L, mut=None):
    """fp32 emulation of csrc/tf_gain.hip -> (B, L) float32"""
    x = np.asarray(x, f32)[:, :L]
    B, T, H = x.shape[0], frames(L), -(-L // HOP)
    G = np.asarray(G, f32)
    if G.ndim == 3 and mut == "gain_of_clip_0":
        G = np.broadcast_to(G[:1], G.shape)
    gt = np.broadcast_to(G, (B,) + G.shape[-2:]).transpose(0, 2, 1)          # (B, T, 513)
    win = window().astype(f32)
    s = frame_index(L, T)
    inside = (s >= 0) & (s < L)
    xw = np.where(inside[None], x[:, np.clip(s, 0, L - 1)], f32(0)) * win
    Xr, Xi = S._fft1024(xw, np.zeros_like(xw), False)
    Yr, Yi = np.zeros_like(Xr), np.zeros_like(Xi)
    Yr[..., :NB], Yi[..., :NB] = gt * Xr[..., :NB], gt * Xi[..., :NB]
    Yr[..., NB:], Yi[..., NB:] = Yr[..., 511:0:-1], -Yi[..., 511:0:-1]
    fr, _ = S._fft1024(Yr, Yi, True)
    contrib = (fr * f32(1.0 / NF)) * win                                       # (B, T, 1024)
    y = np.zeros((B, L), f32)
    for h0 in range(0, H, SLAB_HOPS):
        h1 = min(h0 + SLAB_HOPS, H)
        s0, s1 = h0 * HOP, min(h1 * HOP, L)
        t1 = h1 + HALO
        if mut == "halo_dropped" and h1 < H:
            t1 -= 1                                                            # the slab's last halo frame
        acc = np.zeros((4, B, SLAB), f32)
        for t in range(h0, t1):
            p0 = (t - HALO) * HOP - s0
            n = np.arange(NF)
            ok = (p0 + n >= 0) & (p0 + n < SLAB)
            acc[(t - h0) % 4][:, p0 + n[ok]] += contrib[:, t, ok]
        tot = (((acc[0] + acc[1]) + acc[2]) + acc[3]) * f32(2.0 / 3.0)
        y[:, s0:s1] = tot[:, :s1 - s0]
    return y


# ------------------------------------------------------------------------------------------------------------------ mutants
# name -> (where: "model" or "emulation", case names).  Every listed case is run; the mutant must leave the bound in at least one.
MUTANTS = {
    "hann_symmetric": ("model", ["L6400_ones", "L300_ones"]),
    "frame_offset_2": ("model", ["L6400_rand", "L300_ones"]),
    "no_inv_c": ("model", ["L1024_ones"]),
    "halo_dropped": ("emulation", ["L4999_rand", "L2049_ones"]),
    "nyquist_from_511": ("model", ["L2049_bin512", "L2049_bin511"]),
    "no_conjugation": ("model", ["L1025_rand", "L2049_bin1"]),
    "frame_last_skipped": ("model", ["L300_frame_last", "L2049_frame_last", "L6400_ones"]),
    "gain_of_clip_0": ("model", ["L300_rand_pc", "L2049_bin0_pc"]),
}


_RUNS = {}


def reference(c):
    """(model run, bound) of a case: computed once, shared, never modified"""
    if c.name not in _RUNS:
        i = inputs(c)
        r = model(i.x, i.gain, c.L)
        _RUNS[c.name] = (r, bound(i.x, i.gain, c.L, r))
    return _RUNS[c.name]


def run_case(c, mut=None, where=None):
    """largest |got - model| / bound of the emulation, or of a mutated model / emulation"""
    i = inputs(c)
    r, q = reference(c)
    if where == "model":
        got = model(i.x, i.gain, c.L, mut).y
    else:
        got = emulate(i.x, i.gain, c.L, mut if where == "emulation" else None)
    return ratio(got, r.y, q)
