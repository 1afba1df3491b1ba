"""Shared by tests/test_spectral_bound_host.py (CPU) and tests/test_gpu_spectral_elementwise.py (GPU): a float64 model of the spectral
front end (csrc/stft_mel.hip, the fused route; csrc/mel.hip, the dense-DFT route; csrc/audio_api.hip chooses), its element-wise bound,
an fp32 emulation of each route, mutants and the case table.  No GPU dependency.

MODEL (float64, written from the definition, generic in n_fft / hop / window / bank; `model`):
    ym = fp32(wav * mask)                 the one product the kernels form before a comparison: formed in fp32 here too
    y  = clip(ym, thr[b]) + sigma z       reflect-padded by n_fft / 2, T = 1 + L // hop frames, periodic Hann or rectangular window
    X  = one-sided DFT;  p = |X|^2  or  |X| (+ sigma z_mag);  v = p . fb;  o_raw = 10 log10(max(v, 1e-10)) or v;  o = clamp(o_raw, lo, hi)
  backward, for an explicit cotangent d = dL/do (VJP) or d = -gscale (ref - o) / ||ref - o||_2 (the L2 loss of one clip):
    clamp passes d strictly inside (lo, hi); dB passes it above the floor (times (10 / ln 10) / v); dp = fb dv;
    G = 2 dp X (power) or dp X / |X| with the CLEAN |X| and 0 at |X| = 0; dframe = win . Re sum_k G_k exp(+2 pi i k n / N) over the
    one-sided bins only (no doubling); overlap-add with each padded position folded onto its source sample; the clip passes the
    gradient on -c <= ym <= c; the mask is applied again on store.

BOUND, from the number formats alone (u = 2^-24; `bound`), a componentwise absolute-value propagation of the model.  Every line below
is one line of `bound`; gamma(n) = n u / (1 - n u).  It holds with or without FMA contraction (an FMA has fewer roundings).
  frame     x_n = win_n y_n carries C_IN = 3 roundings (window table, the sample's noise FMA, the product).
  fused DFT five radix-4 Stockham passes.  A pass output is sum_q (+-1, +-i) tw_q v_q: the twiddle is rounded once (relative u in
            modulus), the complex product costs sqrt(2) gamma(2) (Higham, Accuracy and Stability, lemma 3.5), the two levels of complex
            additions (1 + u)^2; the multiplications by +-i are exact.  Per pass (1 + 2 sqrt 2 + 2) u = 5.83 u, the first pass has no
            twiddles (2 u): C_FFT = 2 + 4 * 5.83 = 25.3, taken as 26 to cover the second-order terms.  Every path from x_n to X_k has
            modulus one, so |dX_k| <= (C_FFT + C_IN) u sum_n |win_n y_n| =: (C_FFT + C_IN) u S_f (modulus of the complex error).
  dense DFT a dot product of length n_fft against the table fp32(win cos), fp32(-win sin) (one rounding from float64) on the fp32 MFMA:
            |dX_k| <= (n_fft + 2 + C_IN) u S_f.  ASSUMPTION: the fp32 MFMA rounds every product and every addition to nearest, or fuses
            them; its internal order is free.
  |X|^2     2 |X| bX + bX^2 + 2 u (|X| + bX)^2.
  |X|       bX + (1 + 2 ULP_SQRT) u (|X| + bX); the noise FMA adds u |result|.  ASSUMPTION: device sqrtf within ULP_SQRT = 1 ulp (the
            figure of the HIP math API tables; they are not shipped with the toolchain this was written against, hence an assumption).
  bank      bv = sum_k fb bp + gamma(nnz + 1) sum_k fb (|p| + bp), nnz = non-zero weights of the column (zero weights add exact zeros).
  dB        max(., 1e-10) and clamp are 1-Lipschitz: bo = the larger one-sided change of 10 log10 over [v - bv, v + bv] (floored) plus
            (2 ULP_LOG + 1) u |o|.  ASSUMPTION: device log10f within ULP_LOG = 2 ulp (same source, same caveat).
  loss      diff = ref - o: b = bo + u |diff|; s = sum diff^2 over 1 + 4 + 6 + 3 + nparts roundings deep (square, the lane's frames, the wave
            butterfly, the waves, the partial sums) -- dense: n / 1024 + 14; loss = sqrt(s); inv = gscale / loss.
  d         explicit: exact.  Loss form: product rule on diff * inv, two roundings.
  gates     a mel element within bo of lo or hi, or within bv of the floor, is AMBIGUOUS: for the mel comparison nothing changes (the
            maps are continuous, the Lipschitz bound already covers either branch); for the gradient the whole |dv| of the passing
            branch is added to b(dv).  Cap: at most AMBIG_CAP = 1 % of a case's mel elements, none without a clamp.  A frame the mask
            zeroes entirely has S_f = 0, every bound 0, -100 dB and a zero gradient exactly on both sides: not ambiguous.
  dB'       dv = d (10 / ln 10) / v: constant, quotient, product = 3 roundings, plus |d| c bv / (v (v - bv)).
  bank^T    as the bank, over the non-zero weights of the bin.
  G         power: product rule on 2 dp X, one rounding.  Magnitude: b(dp) + |dp| min(2 bX / |X|, 2) + (3 + 2 ULP_SQRT) u |dp|
            (a unit vector moves by at most twice the relative change; at |X| <= bX either branch of the |X| = 0 rule is covered).
  DFT^T     b(dframe_n) = win_n [sum_k bG + C u sum_k (|G| + bG)], C = C_FFT + 2 (fused) or Kpad + 2 (dense, Kpad = 2 bins rounded up to 32).
  OLA       sum of the n_c contributions that fold onto the sample: sum b + gamma(n_c + 5) sum |.|; the clip gate is exact (same fp32
            product on both sides), the mask one more rounding.

EMULATION (`emulate`): numpy float32 in the kernels' documented order -- radix-4 Stockham with twiddles rounded once, the bank in
increasing bin order, four per-wave accumulators summed in wave order (fused); plain fp32 matrix products, serial candidates (dense).
It validates the bound on the CPU and carries the mutants of the chunk / frame-range / gather logic.  It is not a second oracle.

MUTANTS: `MUTANTS` maps a name to (where it lives, cases); each must leave the bound in at least one element of one listed case.
Three mutants one could ask for are NOT in the table, because no input separates them from the correct code:
  * "clamp gradient passed at o == lo": in float64 o_raw equals a limit only for frames the mask zeroes, where the dB and |X| = 0 rules
    already stop the gradient;
  * "left-reflection override dropped": the chunk is a multiple of the hop in [641, 1280] (or 1280), so the chunk that holds samples
    1 .. 512 is always chunk 0, whose plain frame range starts at frame 0 already -- the override never changes flo.  (The right one
    matters for exactly one sample, when hop divides L and a chunk ends at L - 512: f2560_h512_mag);
  * "10 / ln 10 rounded to 4.3429": a relative change of 1.0e-5 in the gradient.  The worst-case bound of the backward chain is
    (2 (C_FFT + C_IN) + ...) u ~ 1e-5 relative even without any cancellation, so a bound built from the formats alone cannot exclude
    it; `UNSEPARATED` records the ratio it reaches (0.02) so that a sharper bound can pick it up.

CASES: see `CASES`; every case carries `why`, the branch it is there for."""
import math
import zlib
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
C_IN, C_FFT = 3.0, 26.0
ULP_SQRT, ULP_LOG = 1.0, 2.0
FLOOR = 1e-10
C10 = 10.0 / math.log(10.0)
NEG, POS = -3.0e38, 3.0e38
AMBIG_CAP = 0.01
N_MELS = 64
BWD_MAX_CHUNK, FWD_FRAMES = 1280, 16
f32, f64 = np.float32, np.float64


def gamma(n):
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------------------------------ refusal predicates
def fused_route(n_fft, L):
    """audio_api.hip: the fused kernels take n_fft = 1024 (64 mels) and L >= 2048; everything else is dense"""
    return n_fft == 1024 and L >= 2 * n_fft


def refuses_guidance(n_fft, L, power2, has_noise_mag, noise_stride):
    """the fused guidance pair returns an error (and writes nothing) when any of these holds"""
    return (not fused_route(n_fft, L)) or (has_noise_mag and power2) or (noise_stride is not None and noise_stride < L)


def refuses_transform(n_fft, L):
    """reflect padding needs L >= n_fft / 2 + 1"""
    return L < n_fft // 2 + 1


# ------------------------------------------------------------------------------------------------------------------ tables
def window(n_fft, hann, mut=None):
    if not hann:
        return np.ones(n_fft)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / (n_fft - 1 if mut == "hann_symmetric" else n_fft))


def _tri_bank(freqs, pts):
    down = (freqs[:, None] - pts[None, :-2]) / (pts[1:-1] - pts[:-2])[None]
    up = (pts[None, 2:] - freqs[:, None]) / (pts[2:] - pts[1:-1])[None]
    return np.maximum(0.0, np.minimum(down, up))


def bank(kind, bins, sr=16000):
    """(bins, 64) fp32: 'htk' triangles without area normalisation, 'slaney' with it (the two kinds the operators use)"""
    freqs = np.linspace(0.0, sr / 2, bins)
    if kind == "htk":
        mel = np.linspace(0.0, 2595.0 * math.log10(1.0 + (sr / 2) / 700.0), N_MELS + 2)
        return _tri_bank(freqs, 700.0 * (10.0 ** (mel / 2595.0) - 1.0)).astype(f32)
    def hz2mel(f):
        return np.where(f < 1000.0, 3.0 * f / 200.0, 15.0 + np.log(np.maximum(f, 1e-9) / 1000.0) * 27.0 / math.log(6.4))
    def mel2hz(m):
        return np.where(m < 15.0, 200.0 * m / 3.0, 1000.0 * np.exp((m - 15.0) * math.log(6.4) / 27.0))
    pts = mel2hz(np.linspace(0.0, float(hz2mel(np.array(0.45 * sr))), N_MELS + 2))
    return (_tri_bank(freqs, pts) * (2.0 / (pts[2:] - pts[:-2]))[None]).astype(f32)


def dft_matrix(n_fft):
    n, k = np.arange(n_fft)[:, None], np.arange(n_fft // 2 + 1)[None]
    return np.exp(-2j * np.pi * ((n * k) % n_fft) / n_fft)


def frame_index(L, n_fft, hop, T, mut=None):
    """(unfolded, folded) sample index of position n of frame f, (T, n_fft) each"""
    p = np.arange(T)[:, None] * hop + np.arange(n_fft)[None] - n_fft // 2
    s = np.where(p < 0, -p - 1 if mut == "pad_symmetric" else -p, p)
    s = np.where(s >= L, (2 * L - 1 if mut == "right_fold_2L_1" else 2 * (L - 1)) - s, s)
    return p, s


# ------------------------------------------------------------------------------------------------------------------ cases and inputs
def _case(name, why, route, n_fft, L, hop, variant, **kw):
    hann, power2, to_db, lo, hi = {"db": (True, True, True, NEG, POS), "dbc": (True, True, True, 0.0, 20.0),
                                   "mag": (False, False, False, -80.0, 80.0)}[variant]
    c = dict(name=name, why=why, route=route, n_fft=n_fft, L=L, hop=hop, hann=hann, power2=power2, to_db=to_db, lo=lo, hi=hi, B=2,
             bank="htk", mask=None, shared_ref=False, cot=(route == "dense"), sigma=0.0, noise=None, thr=False, Lfull=None, stride=None,
             out_stride=None, gscale=1.0, offset=0)
    c.update(kw)
    c["Lfull"] = c["Lfull"] or L
    c["stride"] = c["stride"] or c["Lfull"]
    c["out_stride"] = c["out_stride"] or c["Lfull"]
    assert route == ("fused" if fused_route(n_fft, L) else "dense") or kw.get("force_dense"), name
    return SimpleNamespace(**c)


def _fused(name, why, L, hop, variant, **kw):
    return _case(name, why, "fused", 1024, L, hop, variant, **kw)


def _dense(name, why, n_fft, L, hop, variant, **kw):
    return _case(name, why, "dense", n_fft, L, hop, variant, **kw)


CASES = [
    # L = 2048: T = 13 at hop 160, one forward workgroup whose waves break early, two backward chunks, the second ragged
    _fused("f2048_h160_db", "minimum length; plain power / dB", 2048, 160, "db"),
    _fused("f2048_h160_dbc", "clamp with both limits populated; shared reference", 2048, 160, "dbc", shared_ref=True, B=3),
    _fused("f2048_h160_mag", "magnitude / linear, rectangular window", 2048, 160, "mag"),
    _fused("f2048_h480_mag", "hop 480 with the magnitude transform", 2048, 480, "mag", gscale=3.0),
    _fused("f2048_h137_db", "odd hop, chunk = 1233", 2048, 137, "db", mask="left"),
    _fused("f2048_h1024_dbc", "no overlap between frames, clamped", 2048, 1024, "dbc"),
    _fused("f2048_h1400_mag", "chunk < hop fallback at the minimum length", 2048, 1400, "mag"),
    _fused("f2049_h480_db", "odd length; hole inside the left reflection zone", 2049, 480, "db", mask="left"),
    _fused("f2049_h160_db_noise", "sample-domain noise, noise row stride > L", 2049, 160, "db", sigma=0.05, noise="sample"),
    _fused("f2049_h1400_dbc", "chunk < hop, clamped, uncovered samples", 2049, 1400, "dbc"),
    _fused("f2049_h137_mag", "hole inside the right reflection zone, magnitude", 2049, 137, "mag", mask="right"),
    _fused("f2207_h137_dbc", "ragged last chunk with an odd hop", 2207, 137, "dbc", B=3),
    _fused("f2207_h1024_db", "gscale != 1 scales the gradient only", 2207, 1024, "db", gscale=0.25),
    _fused("f2207_h480_vjp", "explicit cotangent, slaney bank, hop 480 (caller-owned strided dwav)", 2207, 480, "db", cot=True, bank="slaney",
           out_stride=2215),
    _fused("f2207_h160_mag_thr", "per-clip clip threshold with sample noise", 2207, 160, "mag", thr=True, sigma=0.02, noise="sample"),
    # L = 2560: T = 17 at hop 160, a second forward workgroup that holds one frame
    _fused("f2560_h160_db", "second forward workgroup with one frame; hole in the right zone", 2560, 160, "db", mask="right", B=3),
    _fused("f2560_h480_dbc", "fractional mask", 2560, 480, "dbc", mask="frac", thr=True),
    _fused("f2560_h137_db_tail", "Lfull > L and a row stride larger than Lfull", 2560, 137, "db", Lfull=2592, stride=2601, out_stride=2605),
    _fused("f2560_h1024_db", "shared reference at hop 1024", 2560, 1024, "db", shared_ref=True),
    _fused("f2560_h512_mag", "hop divides L and a chunk ends at L - 512: sample 2047 is reached only through the right-reflection override",
           2560, 512, "mag"),
    _fused("f2560_h1400_mag_nmag", "magnitude-domain noise with chunk < hop", 2560, 1400, "mag", sigma=0.5, noise="mag"),
    _fused("f2561_h1024_mag", "odd length, no overlap, magnitude", 2561, 1024, "mag"),
    _fused("f2561_h160_mag_nmag", "magnitude-domain noise (the divisor stays the clean magnitude)", 2561, 160, "mag", sigma=0.5, noise="mag"),
    _fused("f2561_h480_db_hole", "hole longer than 1024 + hop: whole frames are zero", 2561, 480, "db", mask="long"),
    _fused("f2561_h137_dbc_thr", "left hole with a clip threshold, clamped", 2561, 137, "dbc", mask="left", thr=True),
    # L = 3361: three chunks at hop 160, a true interior chunk
    _fused("f3361_h160_dbc_hole", "three chunks; hole longer than 1024 + hop", 3361, 160, "dbc", mask="long", B=3),
    _fused("f3361_h1400_db", "chunk < hop with three chunks; uncovered samples are exactly 0", 3361, 1400, "db"),
    _fused("f3361_h137_mag", "three chunks, odd hop, magnitude", 3361, 137, "mag"),
    _fused("f3361_h480_db_thr", "per-clip threshold, hop 480", 3361, 480, "db", thr=True),
    _fused("f3361_h480_vjp", "explicit cotangent, slaney bank, three chunks", 3361, 480, "db", cot=True, bank="slaney"),
    _fused("f3361_h1024_dbc_frac", "fractional mask with gscale", 3361, 1024, "dbc", mask="frac", gscale=0.5),
    _fused("f3361_h160_vjp_dbc", "explicit cotangent through the clamp, htk bank", 3361, 160, "dbc", cot=True),
    _fused("f3361_h160_db_tail", "three chunks, Lfull > L, strides", 3361, 160, "db", Lfull=3400, stride=3403, out_stride=3401, shared_ref=True),
    # dense route: n_fft 64 -> Kpad 96 (smallest table, not a multiple of 64); hop 25 breaks the 16-byte alignment of most frames
    _dense("d64_L33_h16", "minimum length: both reflection zones cover the clip", 64, 33, 16, "db"),
    _dense("d64_L64_h25", "unaligned frames", 64, 64, 25, "mag"),
    _dense("d64_L199_h100", "hop > n_fft: uncovered samples", 64, 199, 100, "dbc", B=3),
    _dense("d96_L49_h25", "minimum length, unaligned", 96, 49, 25, "mag"),
    _dense("d96_L96_h100", "hop > n_fft at L = n_fft", 96, 96, 100, "db"),
    _dense("d96_L295_h16", "B T = 57, not a multiple of 64; odd row stride", 96, 295, 16, "dbc", B=3, stride=301),
    _dense("d256_L129_h100", "minimum length", 256, 129, 100, "dbc"),
    _dense("d256_L256_h16", "L = n_fft", 256, 256, 16, "db", B=3),
    _dense("d256_L775_h25", "fast and slow gather paths mixed, odd row stride", 256, 775, 25, "mag", stride=777),
    _dense("d1024_L513_h160", "n_fft 1024 below the fused limit: minimum length", 1024, 513, 160, "db"),
    _dense("d1024_L1600_h480", "n_fft 1024, dense, slaney", 1024, 1600, 480, "dbc", bank="slaney"),
    _dense("d1024_L2047_h137", "one sample below the fused limit", 1024, 2047, 137, "mag"),
    _dense("d1024_L2048_h160", "the dense chain where the fused pair also runs (stft_mag always is dense)", 1024, 2048, 160, "db",
           force_dense=True),
    _dense("d256_L775_h16_off1", "waveform view one sample into its storage: no frame may take the 16-byte path", 256, 775, 16, "db",
           offset=1, stride=780),
]
CASE = {c.name: c for c in CASES}


def _rng(name, tag):
    return np.random.default_rng(zlib.crc32(f"{name}/{tag}".encode()))


def _signal(rng, n, pure_noise):
    t = np.arange(n)
    if pure_noise:
        return 0.3 * rng.standard_normal(n)
    f0, fm = rng.uniform(0.01, 0.2), rng.uniform(0.0005, 0.004)
    return 0.3 * np.sin(2 * np.pi * f0 * t + rng.uniform(0, 6.28)) * (0.6 + 0.4 * np.sin(2 * np.pi * fm * t)) + 0.03 * rng.standard_normal(n)


def _clips(name, tag, B, n):
    rng = _rng(name, tag)
    return np.stack([_signal(rng, n, b == B - 1) for b in range(B)]).astype(f32)


_INPUTS = {}


def inputs(c):
    """everything a case feeds the kernels, fp32 numpy, identical on the host and the GPU side; cached and never modified"""
    if c.name in _INPUTS:
        return _INPUTS[c.name]
    L, B, T, bins = c.L, c.B, 1 + c.L // c.hop, c.n_fft // 2 + 1
    i = SimpleNamespace(T=T, bins=bins, fb=bank(c.bank, bins), mask=None, z=None, zmag=None, thr=None, ref=None, dmel=None, dmag=None)
    i.store = np.concatenate([_clips(c.name, "lead", 1, 4)[0][:c.offset], _clips(c.name, "rows", B, c.stride).ravel()])   # clip b = store[offset + b stride:]
    i.wav = np.stack([i.store[c.offset + b * c.stride: c.offset + b * c.stride + c.Lfull] for b in range(B)])
    if c.mask:
        m = np.ones(L, f32)
        if c.mask == "left":
            m[40:330] = 0.0
        elif c.mask == "right":
            m[L - 400:L - 90] = 0.0
        elif c.mask == "long":
            m[500:500 + 1024 + c.hop + 260] = 0.0
        else:
            m = (0.25 + 0.75 * _rng(c.name, "mask").random(L)).astype(f32)
            m[100:180] = 0.0
        i.mask = m
    if c.noise == "sample":
        i.z = _rng(c.name, "z").standard_normal((B, L + 5)).astype(f32)
    if c.noise == "mag":
        i.zmag = _rng(c.name, "zmag").standard_normal((B, bins, T)).astype(f32)
    if c.thr:
        i.thr = np.linspace(0.12, 0.3, B).astype(f32)                # 0.3-amplitude signals: roughly 35 - 90 % of the samples inside
    if c.cot:
        i.dmel = _rng(c.name, "dmel").standard_normal((B, T, N_MELS)).astype(f32)
    else:
        tgt = SimpleNamespace(**{**vars(c), "name": c.name + "/target", "B": 1 if c.shared_ref else B, "mask": None, "noise": None, "sigma": 0.0,
                                 "thr": False, "cot": True, "stride": c.L, "Lfull": c.L, "offset": 0})
        ti = SimpleNamespace(wav=_clips(c.name, "target", tgt.B, L), mask=None, z=None, zmag=None, thr=None, fb=i.fb, T=T, bins=bins)
        i.ref = model(tgt, ti, forward_only=True).o.astype(f32)
    if c.route == "dense":
        i.dmag = _rng(c.name, "dmag").standard_normal((B, bins, T)).astype(f32)
    _INPUTS[c.name] = i
    return i


# ------------------------------------------------------------------------------------------------------------------ float64 model
def _last_nonzero_cleared(fb, axis):
    out = fb.copy()
    nz = fb != 0
    idx = np.where(nz.any(axis), fb.shape[axis] - 1 - np.argmax(np.flip(nz, axis), axis), -1)
    for j, k in enumerate(idx):
        if k >= 0:
            if axis == 0:
                out[k, j] = 0
            else:
                out[j, k] = 0
    return out


def model(c, i, mut=None, forward_only=False, dmag=None):
    """float64 model -> namespace of every intermediate; dmag: the |X| cotangent of stft_mag_bwd instead of the mel chain"""
    L, B, N, hop = c.L, c.B, c.n_fft, c.hop
    T = L // hop if mut == "frames_L_over_hop" else i.T
    r = SimpleNamespace(T=T)
    w32 = i.wav[:, :L]
    ym = (w32 * i.mask[None]).astype(f32) if i.mask is not None else w32
    r.ym = ym.astype(f64)
    yc = r.ym
    if i.thr is not None:
        cth = i.thr.astype(f64)[:, None]
        yc = np.clip(r.ym, -cth, cth)
        gate_src = w32.astype(f64) if mut == "clip_gate_on_wav" else r.ym
        r.gate = (gate_src >= -cth) & (gate_src <= cth)
    r.p, r.s = frame_index(L, N, hop, T, mut)
    fr = yc[:, r.s]
    if i.z is not None:
        zi = np.clip(r.p + N // 2, 0, i.z.shape[1] - 1) if mut == "noise_at_padded_index" else r.s
        fr = fr + c.sigma * i.z.astype(f64)[:, zi]
    r.win = window(N, c.hann, mut)
    r.xw = fr * r.win
    E = dft_matrix(N)
    r.X = r.xw @ E
    if mut == "drop_dc":
        r.X[..., 0] = 0
    if mut == "drop_nyquist":
        r.X[..., -1] = 0
    r.absX = np.abs(r.X)
    r.pw = r.absX ** 2 if c.power2 else r.absX
    if i.zmag is not None:
        r.pw = r.pw + c.sigma * i.zmag.astype(f64).transpose(0, 2, 1)[:, :T]
    fb = i.fb.astype(f64)
    r.v = r.pw @ (_last_nonzero_cleared(fb, 0) if mut == "fwd_bank_last_bin" else fb)
    r.o_raw = 10.0 * np.log10(np.maximum(r.v, FLOOR)) if c.to_db else r.v
    r.o = np.clip(r.o_raw, c.lo, c.hi)
    if forward_only:
        return r
    if dmag is not None:
        dp = dmag.astype(f64).transpose(0, 2, 1)
        r.dp = dp
        power2 = False
    else:
        power2 = c.power2
        if i.dmel is not None:
            r.d = i.dmel.astype(f64)[:, :T]
        else:
            ref = np.broadcast_to(i.ref.astype(f64), (B,) + i.ref.shape[1:])[:, :T]
            if mut == "shared_ref_per_clip" and i.ref.shape[0] == 1:
                ref = np.concatenate([ref[:1], np.zeros_like(ref[1:])])
            r.diff = ref - r.o
            r.loss = np.sqrt((r.diff ** 2).sum((1, 2)))
            r.inv = np.where(r.loss > 0, c.gscale / np.where(r.loss > 0, r.loss, 1.0), 0.0)
            r.d = -r.diff * r.inv[:, None, None]
            if mut == "gscale_on_loss":
                r.loss = r.loss * c.gscale
        r.clamp_pass = (r.o_raw >= c.lo if mut == "clamp_pass_at_lo" else r.o_raw > c.lo) & (r.o_raw < c.hi)
        r.dv_pass = r.d * ((4.3429 if mut == "c10_rounded" else C10) / np.maximum(r.v, 1e-300)) if c.to_db else r.d
        r.db_pass = (r.v > FLOOR) if c.to_db else np.ones_like(r.v, bool)
        r.dv = np.where(r.clamp_pass & r.db_pass, r.dv_pass, 0.0)
        r.dp = r.dv @ (_last_nonzero_cleared(fb, 1) if mut == "bwd_bank_last_mel" else fb).T
    if power2:
        r.G = 2.0 * r.dp * r.X
    else:
        div = np.abs(r.pw) if mut == "divisor_noisy" else r.absX
        r.G = np.where(r.absX > 0, r.dp / np.where(div > 0, div, 1.0), 0.0) * r.X
    if mut == "two_sided_doubling":
        r.G = r.G.copy()
        r.G[..., 1:-1] *= 2.0
    r.dframe = (r.G @ E.conj().T).real * (1.0 if mut == "no_adjoint_window" else r.win)
    g = np.zeros((B, L))
    r.count = np.zeros(L)
    np.add.at(r.count, r.s.ravel(), 1.0)
    for b in range(B):
        np.add.at(g[b], r.s.ravel(), r.dframe[b].ravel())
    r.g_ola = g
    if i.thr is not None and dmag is None:
        g = g * r.gate
    if i.mask is not None and dmag is None and mut != "mask_not_reapplied":
        g = g * i.mask.astype(f64)[None]
    r.dwav = g
    return r


def mel_padded(r, T):
    """a mutant with fewer frames: the missing ones read as zeros"""
    o = np.zeros((r.o.shape[0], T, r.o.shape[2]))
    o[:, :r.T] = r.o
    return o


# ------------------------------------------------------------------------------------------------------------------ bound
def bound(c, i, r, route=None, dmag=False):
    """element-wise bounds on |kernel - model| for the model run r -> namespace (o, loss, dwav, mag, ambiguous share)"""
    route = route or c.route
    N, L, B = c.n_fft, c.L, c.B
    fb = i.fb.astype(f64)
    kpad = -(-2 * i.bins // 32) * 32
    cA = (C_FFT if route == "fused" else N + 2) + C_IN
    cB = (C_FFT if route == "fused" else kpad) + 2
    q = SimpleNamespace()
    S = np.abs(r.xw).sum(-1, keepdims=True)
    bX = cA * U * S * np.ones_like(r.absX)
    q.mag = bX + (1 + 2 * ULP_SQRT) * U * (r.absX + bX)
    if c.power2 and not dmag:
        bp = 2 * r.absX * bX + bX ** 2 + 2 * U * (r.absX + bX) ** 2
    else:
        bp = q.mag.copy()
    if i.zmag is not None:
        bp = bp + U * (np.abs(r.pw) + bp)
    nnz = (fb != 0).sum(0)[None, None]
    bv = bp @ fb + gamma(nnz + 1) * ((np.abs(r.pw) + bp) @ fb)
    if c.to_db:
        up = 10 * np.log10(np.maximum(r.v + bv, FLOOR)) - r.o_raw
        dn = r.o_raw - 10 * np.log10(np.maximum(r.v - bv, FLOOR))
        bo = np.maximum(up, dn) + (2 * ULP_LOG + 1) * U * (np.abs(r.o_raw) + np.maximum(up, dn))
    else:
        bo = bv
    q.o, q.bv = bo, bv
    amb_clamp = (np.abs(r.o_raw - c.lo) <= bo) | (np.abs(r.o_raw - c.hi) <= bo)
    amb_floor = (np.abs(r.v - FLOOR) <= bv) if c.to_db else np.zeros_like(amb_clamp)
    q.ambiguous = amb_clamp | amb_floor
    q.share = float(q.ambiguous.mean())
    if not hasattr(r, "dp"):
        return q
    if dmag:
        bdp = np.zeros_like(r.dp)
    else:
        if i.dmel is not None:
            bd = np.zeros_like(r.d)
        else:
            bdiff = bo + U * np.abs(r.diff)
            n = r.diff[0].size
            depth = 14 + (-(-i.T // FWD_FRAMES) if route == "fused" else n // 1024)
            s = (r.diff ** 2).sum((1, 2))
            bs = (2 * np.abs(r.diff) * bdiff + bdiff ** 2).sum((1, 2)) + gamma(depth) * ((np.abs(r.diff) + bdiff) ** 2).sum((1, 2))
            root = np.sqrt(s)
            q.loss = np.maximum(np.sqrt(s + bs) - root, root - np.sqrt(np.maximum(s - bs, 0))) + 2 * ULP_SQRT * U * np.sqrt(s + bs)
            low = np.maximum(root - q.loss, 1e-300)
            binv = np.where(root > 0, c.gscale * q.loss / (np.maximum(root, 1e-300) * low) + U * c.gscale / low, 0.0)
            inv, binv = np.abs(r.inv)[:, None, None], binv[:, None, None]
            bd = bdiff * inv + np.abs(r.diff) * binv + bdiff * binv + 2 * U * (np.abs(r.diff) + bdiff) * (inv + binv)
        if c.to_db:                                         # on the passing branch the kernel's own v is above the floor
            vs, vlow = np.maximum(r.v, FLOOR), np.maximum(r.v - bv, FLOOR)
            bpass = bd * C10 / vlow + np.abs(r.d) * C10 * bv / (vs * vlow) + 3 * U * (np.abs(r.dv_pass) + bd * C10 / vlow)
        else:
            bpass = bd
        bdv = np.where(q.ambiguous, np.abs(r.dv_pass) + bpass, np.where(r.clamp_pass & r.db_pass, bpass, 0.0))
        nm = (fb != 0).sum(1)[None, None]
        bdp = bdv @ fb.T + gamma(nm + 1) * ((np.abs(r.dv) + bdv) @ fb.T)
    adp = np.abs(r.dp)
    if c.power2 and not dmag:
        bG = 2 * (adp * bX + bdp * r.absX + bdp * bX) + U * 2 * (adp + bdp) * (r.absX + bX)
    else:
        turn = np.minimum(2 * bX / np.maximum(r.absX, 1e-300), 2.0)
        turn = np.where(bX == 0, 0.0, turn)
        bG = bdp + adp * turn + (3 + 2 * ULP_SQRT) * U * (adp + bdp)
    sumG = (np.abs(r.G) + bG).sum(-1, keepdims=True)
    bframe = r.win[None, None] * (bG.sum(-1, keepdims=True) + cB * U * sumG)
    bg, ag = np.zeros((B, L)), np.zeros((B, L))
    for b in range(B):
        np.add.at(bg[b], r.s.ravel(), bframe[b].ravel())
        np.add.at(ag[b], r.s.ravel(), np.abs(r.dframe[b]).ravel())
    bg = bg + gamma(r.count + 5)[None] * (ag + bg)
    if not dmag:
        if i.thr is not None:
            bg = bg * r.gate
        if i.mask is not None:
            bg = bg * np.abs(i.mask.astype(f64))[None]
    q.dwav = bg
    return q


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation
def _fft1024(re, im, inverse):
    """radix-4 Stockham, five in-place passes over (..., 1024) float32 pairs, in the kernel's order (no FMA)"""
    ang = 2.0 * np.pi * np.arange(1024) / 1024
    twr, twi = np.cos(ang).astype(f32), (-np.sin(ang)).astype(f32)
    if inverse:
        twi = -twi
    j = np.arange(256)
    for NS in (1, 4, 16, 64, 256):
        k = j & (NS - 1)
        vr = [re[..., j + 256 * qq] for qq in range(4)]
        vi = [im[..., j + 256 * qq] for qq in range(4)]
        if NS > 1:
            for qq in range(1, 4):
                wr, wi = twr[qq * k * (256 // NS)], twi[qq * k * (256 // NS)]
                vr[qq], vi[qq] = vr[qq] * wr - vi[qq] * wi, vr[qq] * wi + vi[qq] * wr
        ar, ai, br, bi = vr[0] + vr[2], vi[0] + vi[2], vr[0] - vr[2], vi[0] - vi[2]
        cr, ci, d0r, d0i = vr[1] + vr[3], vi[1] + vi[3], vr[1] - vr[3], vi[1] - vi[3]
        dr, di = (-d0i, d0r) if inverse else (d0i, -d0r)
        outs = ((ar + cr, ai + ci), (br + dr, bi + di), (ar - cr, ai - ci), (br - dr, bi - di))
        j0 = ((j - k) << 2) + k
        re, im = np.empty_like(re), np.empty_like(im)
        for qq in range(4):
            re[..., j0 + qq * NS], im[..., j0 + qq * NS] = outs[qq]
    return re, im


def _fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _tail32(c, v):
    o = f32(10.0) * np.log10(np.maximum(v, f32(1e-10))).astype(f32) if c.to_db else v
    return o, np.minimum(np.maximum(o, f32(c.lo)), f32(c.hi))


def _seq_dot(w, x, order_axis_len):
    """acc += w[k] * x[..., k] for k in increasing order, fp32"""
    acc = np.zeros(x.shape[:-1] + (w.shape[1],), f32)
    for k in range(order_axis_len):
        if w[k].any():
            acc = acc + w[k][None, None] * x[..., k:k + 1]
    return acc


def _load32(c, i, s, mut=None, p=None):
    y = i.wav[:, :c.L]
    if i.mask is not None:
        y = y * i.mask[None]
    if i.thr is not None:
        y = np.clip(y, -i.thr[:, None], i.thr[:, None])
    fr = y[:, s]
    if i.z is not None:
        fr = _fma(f32(c.sigma), i.z[:, s], fr)
    return fr


def emulate(c, i, mut=None, route=None, dmag=None):
    """fp32 emulation of one route -> namespace(o, loss, dwav, mag); `mut`: a mutant of the route's own logic"""
    route = route or c.route
    return (_emulate_fused if route == "fused" else _emulate_dense)(c, i, mut, dmag)


def _emulate_fused(c, i, mut, dmag):
    L, B, hop, T = c.L, c.B, c.hop, i.T
    e = SimpleNamespace()
    p, s = frame_index(L, 1024, hop, T)
    win = window(1024, c.hann).astype(f32)
    xr = _load32(c, i, s) * win
    Xr, Xi = _fft1024(xr, np.zeros_like(xr), False)
    Xr, Xi = Xr[..., :513], Xi[..., :513]
    pw = Xr * Xr + Xi * Xi
    if not c.power2:
        pw = np.sqrt(pw)
    clean = pw
    if i.zmag is not None:
        pw = _fma(f32(c.sigma), i.zmag.transpose(0, 2, 1), pw)
    v = _seq_dot(i.fb, pw, 513)
    o_raw, o = _tail32(c, v)
    e.o = o
    if i.dmel is not None:
        d = i.dmel
    else:
        ref = np.broadcast_to(i.ref, (B, T, N_MELS))
        diff = ref - o
        sq = np.zeros((B, -(-T // FWD_FRAMES), 4, N_MELS), f32)
        for f in range(T):
            sq[:, f // FWD_FRAMES, f % 4] += diff[:, f] * diff[:, f]
        w = sq
        while w.shape[-1] > 1:
            w = w[..., :w.shape[-1] // 2] + w[..., w.shape[-1] // 2:]
        w = w[..., 0]
        part = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
        ssum = np.zeros(B, f32)
        for k in range(part.shape[1]):
            ssum = ssum + part[:, k]
        e.loss = np.sqrt(ssum)
        inv = np.where(e.loss > 0, f32(c.gscale) / np.where(e.loss > 0, e.loss, f32(1)), f32(0)).astype(f32)
        d = -(ref - o) * inv[:, None, None]
    d = np.where((o_raw < f32(c.lo)) | (o_raw > f32(c.hi)), f32(0), d)
    if c.to_db:
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where(v > f32(1e-10), d * (f32(4.342944819032518) / v), f32(0)).astype(f32)
    dp = np.zeros((B, T, 513), f32)
    for m in range(N_MELS):                                  # increasing mel column order over the non-zero weights of each bin
        col = i.fb[:, m]
        if col.any():
            dp = dp + col[None, None] * d[..., m:m + 1]
    if c.power2:
        Gr, Gi = f32(2) * dp * Xr, f32(2) * dp * Xi
    else:
        mag = np.sqrt(Xr * Xr + Xi * Xi) if i.zmag is not None else clean
        with np.errstate(divide="ignore", invalid="ignore"):
            cc = np.where(mag > 0, dp / mag, f32(0)).astype(f32)
        Gr, Gi = cc * Xr, cc * Xi
    br, bi = np.zeros((B, T, 1024), f32), np.zeros((B, T, 1024), f32)
    br[..., :513], bi[..., :513] = Gr, Gi
    fr, _ = _fft1024(br, bi, True)
    contrib = fr * win
    chunk = (BWD_MAX_CHUNK // hop) * hop
    if chunk < hop:
        chunk = BWD_MAX_CHUNK
    g = np.zeros((B, L), f32)
    for ci, s0 in enumerate(range(0, L, chunk)):
        s1 = min(s0 + chunk, L)
        a0 = s0 + 512 - 1023
        flo = 0 if a0 <= 0 else (a0 + hop - 1) // hop
        fhi = min(T - 1, (s1 - 1 + 512) // hop)
        if s0 <= 512 and s1 > 1 and mut != "no_left_override":
            flo = 0
        if s1 - 1 >= L - 1 - 512 and s0 <= L - 2 and mut != "no_right_override":
            fhi = T - 1
        if mut == "fhi_short" and ci == 0:
            fhi -= 1
        if mut == "flo_late" and ci == 1:
            flo += 1
        acc = np.zeros((4, B, s1 - s0), f32)
        for f in range(flo, fhi + 1):
            wv = (f - flo) % 4
            sr = p[f]
            for ps in range(3):
                if ps == 0:
                    tgt, ok = sr, (sr >= 0) & (sr < L)
                elif ps == 1:
                    tgt, ok = -sr, sr < 0
                else:
                    tgt, ok = 2 * (L - 1) - sr, sr >= L
                ok = ok & (tgt >= s0) & (tgt < s1)
                if ok.any():
                    acc[wv][:, tgt[ok] - s0] += contrib[:, f, ok]
        g[:, s0:s1] = ((acc[0] + acc[1]) + acc[2]) + acc[3]
    if i.thr is not None:
        y = i.wav[:, :L] * i.mask[None] if i.mask is not None else i.wav[:, :L]
        g = np.where((y >= -i.thr[:, None]) & (y <= i.thr[:, None]), g, f32(0))
    if i.mask is not None:
        g = g * i.mask[None]
    e.dwav = g
    return e


def _emulate_dense(c, i, mut, dmag):
    L, B, N, hop, T, bins = c.L, c.B, c.n_fft, c.hop, i.T, i.bins
    e = SimpleNamespace()
    p, s = frame_index(L, N, hop, T)
    if mut == "gather_fast_on_edge":                       # the unfolded index read straight from storage
        flat = i.store
        idx = np.clip(c.offset + np.arange(B)[:, None, None] * c.stride + p[None], 0, flat.size - 1)
        fr = flat[idx]
    else:
        fr = i.wav[:, :L][:, s]
    n, k = np.arange(N)[:, None], np.arange(bins)[None]
    ang = 2.0 * np.pi * ((n * k) % N) / N
    w = window(N, c.hann)[:, None]
    tc, ts = (w * np.cos(ang)).astype(f32), (-w * np.sin(ang)).astype(f32)
    Xr, Xi = fr @ tc, fr @ ts
    m2 = Xr * Xr + Xi * Xi
    e.mag = np.sqrt(m2).transpose(0, 2, 1)
    if dmag is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            cc = np.where(np.sqrt(m2) > 0, dmag.transpose(0, 2, 1) / np.sqrt(m2), f32(0)).astype(f32)
        Gr, Gi = cc * Xr, cc * Xi
    else:
        pw = m2 if c.power2 else np.sqrt(m2)
        v = _seq_dot(i.fb, pw, bins)
        o_raw, e.o = _tail32(c, v)
        d = np.where((o_raw < f32(c.lo)) | (o_raw > f32(c.hi)), f32(0), i.dmel)
        if c.to_db:
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.where(v > f32(1e-10), d * (f32(4.342944819032518) / v), f32(0)).astype(f32)
        dp = np.zeros((B, T, bins), f32)
        for m in range(N_MELS):
            col = i.fb[:, m]
            if col.any():
                dp = dp + col[None, None] * d[..., m:m + 1]
        if c.power2:
            Gr, Gi = f32(2) * dp * Xr, f32(2) * dp * Xi
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                cc = np.where(np.sqrt(m2) > 0, dp / np.sqrt(m2), f32(0)).astype(f32)
            Gr, Gi = cc * Xr, cc * Xi
    df = Gr @ tc.T + Gi @ ts.T                               # (B, T, N)
    pad = N // 2
    g = np.zeros((B, L), f32)
    for t in range(L):
        cand = [t + pad]
        if 1 <= t <= pad:
            cand.append(pad - t)
        q = 2 * (L - 1) + pad - t
        if L + pad <= q < L + 2 * pad and mut != "ola_no_right_candidate":
            cand.append(q)
        acc = np.zeros(B, f32)
        for pp in cand:
            f0 = 0 if pp - (N - 1) <= 0 else (pp - (N - 1) + hop - 1) // hop
            for f in range(f0, min(pp // hop, T - 1) + 1):
                acc = acc + df[:, f, pp - f * hop]
        g[:, t] = acc
    e.dwav = g
    return e


def melscale_model(mag, fb, lo, hi):
    """float64 MelScale on a given magnitude (B, bins, T) -> (value, bound)"""
    m = mag.astype(f64).transpose(0, 2, 1)
    fb = fb.astype(f64)
    v = m @ fb
    return np.clip(v, lo, hi), gamma((fb != 0).sum(0)[None, None] + 1) * (np.abs(m) @ fb)


# ------------------------------------------------------------------------------------------------------------------ comparison, mutants
def ratio(got, want, bnd):
    """largest |got - want| / bound; an element with a zero bound must match exactly (ratio inf otherwise); NaN counts as inf"""
    err = np.abs(np.asarray(got, f64) - want)
    if not np.all(np.isfinite(err)):
        return math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bnd)
    return float(np.max(r)) if r.size else 0.0


# name -> (where: "model" or "emulation", case names).  Every listed case is run; the mutant must leave the bound in at least one.
MUTANTS = {
    "pad_symmetric": ("model", ["f2048_h160_db", "d64_L33_h16"]),
    "right_fold_2L_1": ("model", ["f2048_h160_db", "d96_L49_h25"]),
    "frames_L_over_hop": ("model", ["f2560_h160_db"]),
    "hann_symmetric": ("model", ["f2048_h160_db"]),
    "no_adjoint_window": ("model", ["f2048_h160_db"]),
    "fhi_short": ("emulation", ["f3361_h137_mag", "f2048_h160_mag"]),
    "flo_late": ("emulation", ["f3361_h137_mag", "f2048_h160_db"]),
    "no_right_override": ("emulation", ["f2560_h512_mag"]),
    "bwd_bank_last_mel": ("model", ["f2048_h160_db"]),
    "fwd_bank_last_bin": ("model", ["f2048_h160_db"]),
    "two_sided_doubling": ("model", ["f2048_h160_db"]),
    "drop_dc": ("model", ["d64_L64_h25"]),                 # the triangular banks weigh DC and Nyquist with 0: only stft_mag sees them
    "drop_nyquist": ("model", ["d64_L64_h25"]),
    "noise_at_padded_index": ("model", ["f2049_h160_db_noise"]),
    "mask_not_reapplied": ("model", ["f2560_h480_dbc"]),
    "clip_gate_on_wav": ("model", ["f2560_h480_dbc"]),
    "divisor_noisy": ("model", ["f2561_h160_mag_nmag"]),
    "gscale_on_loss": ("model", ["f2207_h1024_db"]),
    "shared_ref_per_clip": ("model", ["f2048_h160_dbc"]),
    "gather_fast_on_edge": ("emulation", ["d256_L775_h25"]),
    "ola_no_right_candidate": ("emulation", ["d256_L775_h25"]),
}


UNSEPARATED = {"c10_rounded": ("model", ["f2207_h480_vjp", "f3361_h480_vjp"])}


def run_case(c, mut=None, where=None):
    """model + bound (never mutated) against the emulation, or against a mutated model / emulation -> {kind: ratio}"""
    i = inputs(c)
    r = model(c, i)
    q = bound(c, i, r)
    if where == "model":
        m = model(c, i, mut)
        got = SimpleNamespace(o=mel_padded(m, i.T), dwav=m.dwav, loss=getattr(m, "loss", None))
    else:
        got = emulate(c, i, mut if where == "emulation" else None)
    out = {"mel": ratio(got.o, r.o, q.o), "dwav": ratio(got.dwav, r.dwav, q.dwav)}
    if i.dmel is None and getattr(got, "loss", None) is not None:
        out["loss"] = ratio(got.loss, r.loss, q.loss)
    if c.route == "dense" and where != "emulation":
        rm = model(c, i, dmag=i.dmag)
        qm = bound(c, i, rm, dmag=True)
        if where == "model":
            mm = model(c, i, mut, dmag=i.dmag)
            em = SimpleNamespace(mag=mm.absX.transpose(0, 2, 1), dwav=mm.dwav)
        else:
            em = emulate(c, i, dmag=i.dmag)
        out["mag"] = ratio(em.mag, rm.absX.transpose(0, 2, 1), qm.mag.transpose(0, 2, 1))
        out["dmag"] = ratio(em.dwav, rm.dwav, qm.dwav)
    return out, q
