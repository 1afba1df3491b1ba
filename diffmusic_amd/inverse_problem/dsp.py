"""Host-side DSP tables (built once, uploaded to the HIP library): torchaudio-compatible HTK mel
filterbank (norm=None) and the sinc-hann polyphase resampling kernel."""
import math
import numpy as np


def melscale_fbanks(n_freqs=513, f_min=0.0, f_max=8000.0, n_mels=64, sample_rate=16000):
    """(n_freqs, n_mels) float32 triangular filters, HTK mel scale, no area normalisation."""
    all_freqs = np.linspace(0.0, sample_rate // 2, n_freqs, dtype=np.float32)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = np.linspace(m_min, m_max, n_mels + 2, dtype=np.float32)
    f_pts = (700.0 * (np.power(np.float32(10.0), m_pts / np.float32(2595.0)) - 1.0)).astype(np.float32)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return np.maximum(0.0, np.minimum(down, up)).astype(np.float32)


def sinc_resample_kernel(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """Returns (kernel (new, taps) float32, width, orig, new) after gcd reduction."""
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = (np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx) * base
    t = np.clip(t, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kern = np.where(t == 0, 1.0, np.sin(t) / np.where(t == 0, 1.0, t)) * window * (base / orig)
    return kern.astype(np.float32), width, orig, new


def threshold_for_sdr(clean, sdr_db, tol_db=1e-9, max_iter=200):
    """Per-clip hard-clip threshold c for which the clipped signal has the asked input SDR,
        10 log10(||x||^2 / ||x - clip(x, c)||^2) = sdr_db,
    the way declipping benchmarks state their difficulty (1 / 3 / 5 / 10 dB).  clean: (B, L) or (L,) array or tensor -> (B,) float64
    numpy array.  The SDR rises monotonically with c (0 dB at c = 0, unbounded at c = max |x|), so this is a bisection in float64 on the
    host; it runs once per clip when the measurement is built."""
    x = clean.detach().cpu().numpy() if hasattr(clean, "detach") else np.asarray(clean)
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    sdr_db = float(sdr_db)
    if not sdr_db > 0.0 or not math.isfinite(sdr_db):
        raise ValueError(f"sdr_db = {sdr_db!r}: a positive finite number (clipping at c > 0 always leaves more than 0 dB)")
    out = np.empty(x.shape[0], dtype=np.float64)
    for b, row in enumerate(x):
        a = np.abs(row)
        energy = float(np.dot(a, a))
        if not energy > 0.0 or not math.isfinite(energy):
            raise ValueError(f"clip {b} is all zero (or not finite): no threshold gives it an SDR")

        def sdr(c):
            r = np.maximum(a - c, 0.0)
            return 10.0 * math.log10(energy / max(float(np.dot(r, r)), 1e-300))

        lo, hi = 0.0, float(a.max())                          # sdr(lo) = 0 dB < sdr_db < sdr(hi)
        for _ in range(max_iter):
            mid = 0.5 * (lo + hi)
            v = sdr(mid)
            if abs(v - sdr_db) <= tol_db or mid in (lo, hi):
                break
            if v < sdr_db:
                lo = mid
            else:
                hi = mid
        out[b] = mid
    return out


# ---- time-frequency masking (TimeFrequencyMaskOperator; csrc/tf_gain.hip): n_fft 1024, hop 256, frame t starts at sample (t - 3) * 256
TF_N_FFT, TF_HOP, TF_BINS = 1024, 256, 513


def tf_frames(length):
    """Frames of the time-frequency grid of a clip of `length` samples: T = ceil(length / 256) + 3."""
    length = int(length)
    if length < 1:
        raise ValueError(f"length = {length!r}: at least one sample")
    return -(-length // TF_HOP) + TF_N_FFT // TF_HOP - 1


def tf_gain_grid(length, sample_rate, boxes, base=1.0):
    """(513, T) fp32 gain grid: `base` everywhere, overwritten in order by boxes (f_lo_hz, f_hi_hz, t0_s, t1_s, gain); a None bound means
    "to the edge".  Bin k belongs to a box when f_lo <= k * sample_rate / 1024 <= f_hi, frame t when its centre
    ((t - 3) * 256 + 512) / sample_rate lies in [t0, t1)."""
    T = tf_frames(length)
    grid = np.full((TF_BINS, T), base, dtype=np.float32)
    if not np.isfinite(grid).all():
        raise ValueError(f"base = {base!r}: a finite number")
    freq = np.arange(TF_BINS, dtype=np.float64) * float(sample_rate) / TF_N_FFT
    centre = ((np.arange(T, dtype=np.float64) - (TF_N_FFT // TF_HOP - 1)) * TF_HOP + TF_N_FFT // 2) / float(sample_rate)
    for box in boxes:
        if len(box) != 5:
            raise ValueError(f"box {box!r}: (f_lo_hz, f_hi_hz, t0_s, t1_s, gain)")
        f_lo, f_hi, t0, t1, gain = box
        if not math.isfinite(float(gain)):
            raise ValueError(f"box {box!r}: a finite gain")
        rows = (freq >= (-math.inf if f_lo is None else float(f_lo))) & (freq <= (math.inf if f_hi is None else float(f_hi)))
        cols = (centre >= (-math.inf if t0 is None else float(t0))) & (centre < (math.inf if t1 is None else float(t1)))
        grid[np.ix_(rows, cols)] = np.float32(gain)
    return grid


def hum_boxes(f0_hz, harmonics=1, width_hz=32.0, gain=0.0):
    """Boxes for `tf_gain_grid` that remove mains hum: bands of `width_hz` centred on f0, 2 f0, ..., harmonics * f0, over the whole clip.
    The bins are sample_rate / 1024 apart (15.6 Hz at 16 kHz): a band narrower than that may hold no bin."""
    f0_hz, harmonics, width_hz = float(f0_hz), int(harmonics), float(width_hz)
    if not (math.isfinite(f0_hz) and f0_hz > 0) or harmonics < 1 or not (math.isfinite(width_hz) and width_hz >= 0):
        raise ValueError(f"hum_boxes({f0_hz!r}, {harmonics!r}, {width_hz!r}): a positive frequency, at least one harmonic, a width >= 0")
    return [(m * f0_hz - 0.5 * width_hz, m * f0_hz + 0.5 * width_hz, None, None, float(gain)) for m in range(1, harmonics + 1)]


# ---- codec restoration (CodecOperator; csrc/mdct_quant.hip): MDCT with N = 512 coefficients per frame, frame length 1024, hop 512, sine
# window, frame t starts at sample (t - 1) * 512; coefficient k sits at (k + 1/2) * sample_rate / 1024
MDCT_N = 512


def mdct_frames(length):
    """Frames of the MDCT of a clip of `length` samples: T = ceil(length / 512) + 1."""
    length = int(length)
    if length < 1:
        raise ValueError(f"length = {length!r}: at least one sample")
    return -(-length // MDCT_N) + 1


def _mdct_basis():
    """(1024, 512) float64: sqrt(2 / N) w[n] cos(pi / N (n + 1/2 + N / 2)(k + 1/2)), the windowed, scaled MDCT basis of one frame."""
    n, k = np.arange(2 * MDCT_N, dtype=np.float64)[:, None], np.arange(MDCT_N, dtype=np.float64)[None]
    w = np.sin(np.pi * (n + 0.5) / (2 * MDCT_N))
    return math.sqrt(2.0 / MDCT_N) * w * np.cos(np.pi / MDCT_N * (n + 0.5 + MDCT_N / 2) * (k + 0.5))


def mdct(audio):
    """audio (..., L) -> (..., 512, T) float64 MDCT coefficients from the definition, the clip zero outside [0, L) (host; not on the step path)."""
    x = np.asarray(audio, dtype=np.float64)
    L = x.shape[-1]
    T = mdct_frames(L)
    pad = np.zeros(x.shape[:-1] + ((T + 1) * MDCT_N,))
    pad[..., MDCT_N:MDCT_N + L] = x                                    # frame t starts at (t - 1) 512: shift by one hop
    fr = np.stack([pad[..., t * MDCT_N:t * MDCT_N + 2 * MDCT_N] for t in range(T)], axis=-2)      # (..., T, 1024)
    return np.swapaxes(fr @ _mdct_basis(), -1, -2)


def imdct(coeffs, length):
    """coeffs (..., 512, T) -> (..., length) float64: the transpose of `mdct` (the same cosines, the window, overlap-add, cropped to the clip);
    with T = mdct_frames(length), imdct(mdct(x), L) = x."""
    c = np.asarray(coeffs, dtype=np.float64)
    T = mdct_frames(length)
    if c.shape[-2:] != (MDCT_N, T):
        raise ValueError(f"coeffs have shape {c.shape}: (..., {MDCT_N}, {T}) for a clip of {length} samples")
    fr = np.swapaxes(c, -1, -2) @ _mdct_basis().T                      # (..., T, 1024)
    out = np.zeros(c.shape[:-2] + ((T + 1) * MDCT_N,))
    for t in range(T):
        out[..., t * MDCT_N:t * MDCT_N + 2 * MDCT_N] += fr[..., t, :]
    return out[..., MDCT_N:MDCT_N + int(length)]


def codec_bands(sample_rate, n=21):
    """n + 1 increasing band edges over the 512 coefficients (edge[0] = 0, edge[n] = 512) on a Bark-like scale: equal steps of
    z(f) = 13 atan(0.00076 f) + 3.5 atan((f / 7500)^2) up to sample_rate / 2, every band at least one coefficient wide."""
    n = int(n)
    if not (math.isfinite(float(sample_rate)) and float(sample_rate) > 0) or not 1 <= n <= MDCT_N:
        raise ValueError(f"codec_bands({sample_rate!r}, {n!r}): a positive rate and 1 .. {MDCT_N} bands")
    f = (np.arange(MDCT_N + 1, dtype=np.float64)) * float(sample_rate) / (2 * MDCT_N)
    z = 13.0 * np.arctan(0.00076 * f) + 3.5 * np.arctan((f / 7500.0) ** 2)
    edges = np.searchsorted(z, np.linspace(0.0, z[-1], n + 1)).astype(np.int64)
    edges[0], edges[-1] = 0, MDCT_N
    for i in range(1, n + 1):                                          # at least one coefficient per band, from the low end
        edges[i] = max(edges[i], edges[i - 1] + 1)
    for i in range(n - 1, -1, -1):                                     # and without running past 512 at the high end
        edges[i] = min(edges[i], edges[i + 1] - 1)
    return edges


def _codec_cutoff(sample_rate, cutoff_hz):
    """First discarded coefficient: those whose centre (k + 1/2) sample_rate / 1024 lies above the cut-off (None: none)."""
    if cutoff_hz is None:
        return MDCT_N
    cutoff_hz = float(cutoff_hz)
    if not (math.isfinite(cutoff_hz) and cutoff_hz > 0):
        raise ValueError(f"cutoff_hz = {cutoff_hz!r}: a positive finite frequency, or None")
    centre = (np.arange(MDCT_N, dtype=np.float64) + 0.5) * float(sample_rate) / (2 * MDCT_N)
    return int(np.searchsorted(centre, cutoff_hz, side="right"))


def codec_step_grid(length, sample_rate, step_db, cutoff_hz=None, tilt_db_per_octave=0.0):
    """(512, T) fp32 step grid, the same in every frame: D = 10^(step_db / 20) at 1 kHz, tilted by `tilt_db_per_octave` (coarser towards the
    top when positive), +inf for the coefficients above `cutoff_hz`."""
    T = mdct_frames(length)
    step_db, tilt = float(step_db), float(tilt_db_per_octave)
    if not (math.isfinite(step_db) and abs(step_db) <= 200 and math.isfinite(tilt) and abs(tilt) <= 48):
        raise ValueError(f"codec_step_grid: step_db = {step_db!r} (finite, at most 200 in magnitude), tilt_db_per_octave = {tilt!r} (at most 48)")
    centre = (np.arange(MDCT_N, dtype=np.float64) + 0.5) * float(sample_rate) / (2 * MDCT_N)
    col = 10.0 ** ((step_db + tilt * np.log2(centre / 1000.0)) / 20.0)
    col[_codec_cutoff(sample_rate, cutoff_hz):] = np.inf
    return np.repeat(col.astype(np.float32)[:, None], T, axis=1)


def codec_steps_for_nmr(audio, sample_rate, nmr_db, cutoff_hz=None, bands=21, floor=1e-10):
    """(512, T) or (B, 512, T) fp32 step grid for audio (L,) or (B, L), the one a codec's rate loop would choose: per band of `codec_bands`
    and frame D = sqrt(12 E 10^(-nmr_db / 10)), E the band's mean coefficient power in that frame (floored), so that the quantisation noise
    D^2 / 12 of a uniform quantiser sits `nmr_db` below the band; +inf above `cutoff_hz`."""
    nmr_db = float(nmr_db)
    if not (math.isfinite(nmr_db) and abs(nmr_db) <= 200):
        raise ValueError(f"nmr_db = {nmr_db!r}: a finite number, at most 200 in magnitude")
    x = np.asarray(audio, dtype=np.float64)
    if x.ndim not in (1, 2) or not np.isfinite(x).all():
        raise ValueError(f"audio has shape {x.shape}: (L,) or (B, L), finite")
    C = mdct(x)
    edges = codec_bands(sample_rate, bands)
    D = np.empty_like(C)
    for lo, hi in zip(edges[:-1], edges[1:]):
        E = np.maximum((C[..., lo:hi, :] ** 2).mean(axis=-2, keepdims=True), float(floor))
        D[..., lo:hi, :] = np.sqrt(12.0 * E * 10.0 ** (-nmr_db / 10.0))
    D[..., _codec_cutoff(sample_rate, cutoff_hz):, :] = np.inf
    return D.astype(np.float32)


# ---- blind equalisation (BlindEqualizationOperator; csrc/tf_eq.hip): a gain per bin, constant in time; bin k sits at k * sample_rate / 1024
def eq_curve(sample_rate, points):
    """(513,) fp32 gain curve through (frequency_hz, gain_db) breakpoints: linear in dB over log-frequency between them, flat beyond the
    first and the last (DC included).  Frequencies positive and strictly increasing."""
    pts = [(float(f), float(db)) for f, db in points]
    if not pts or not all(math.isfinite(f) and f > 0 and math.isfinite(db) for f, db in pts) or \
            any(b[0] <= a[0] for a, b in zip(pts, pts[1:])):
        raise ValueError(f"eq_curve points {points!r}: at least one (hz, dB) pair, finite, frequencies positive and strictly increasing")
    freq = np.arange(TF_BINS, dtype=np.float64) * float(sample_rate) / TF_N_FFT
    logf = np.log(np.maximum(freq, pts[0][0]))               # below the first breakpoint (and at DC): its value
    db = np.interp(logf, np.log([f for f, _ in pts]), [d for _, d in pts])
    return (10.0 ** (db / 20.0)).astype(np.float32)


def lowpass_curve(sample_rate, cutoff_hz, order=4):
    """(513,) fp32 magnitude of a Butterworth low-pass: 1 / sqrt(1 + (f / cutoff_hz)^(2 * order)), f = k * sample_rate / 1024."""
    cutoff_hz, order = float(cutoff_hz), int(order)
    if not (math.isfinite(cutoff_hz) and cutoff_hz > 0) or order < 1:
        raise ValueError(f"lowpass_curve({cutoff_hz!r}, order={order!r}): a positive cut-off and an order >= 1")
    freq = np.arange(TF_BINS, dtype=np.float64) * float(sample_rate) / TF_N_FFT
    return (1.0 / np.sqrt(1.0 + (freq / cutoff_hz) ** (2 * order))).astype(np.float32)


# ---- de-compression (DynamicRangeOperator; csrc/drc.hip): a compressor whose sidechain runs on blocks of 64 samples
DRC_BLOCK = 64


def drc_coeffs(sample_rate, attack_ms, release_ms):
    """(aA, aR) as np.float32: the per-block coefficients 1 - exp(-64 / (sample_rate * t)) of the attack / release follower, computed in
    float64 and rounded once -- the constants the kernels and the tests' model share."""
    sample_rate, attack_ms, release_ms = float(sample_rate), float(attack_ms), float(release_ms)
    if not (math.isfinite(sample_rate) and sample_rate > 0):
        raise ValueError(f"sample_rate = {sample_rate!r}: a positive finite rate")
    out = []
    for name, ms in (("attack_ms", attack_ms), ("release_ms", release_ms)):
        if not (math.isfinite(ms) and ms > 0):
            raise ValueError(f"{name} = {ms!r}: a positive finite time in milliseconds")
        a = np.float32(-math.expm1(-DRC_BLOCK / (sample_rate * ms * 1e-3)))
        if not 0.0 < float(a) <= 1.0:
            raise ValueError(f"{name} = {ms!r}: its per-block coefficient {float(a)!r} rounds outside (0, 1] -- too long for blocks of "
                             f"{DRC_BLOCK} samples at {sample_rate} Hz")
        out.append(a)
    return out[0], out[1]


def drc_static_curve(level_db, threshold_db, ratio, knee_db):
    """Gain reduction c >= 0 in dB of a compressor's static curve at `level_db` (float64 array): with d = level - threshold, k = 1 - 1 / ratio
    and knee width W, c = 0 where 2 d < -W, k (d + W / 2)^2 / (2 W) where 2 d <= W, and k d above (ratio = inf: a limiter)."""
    threshold_db, ratio, knee_db = float(threshold_db), float(ratio), float(knee_db)
    if math.isnan(ratio) or ratio < 1:
        raise ValueError(f"ratio = {ratio!r}: at least 1 (inf = a limiter)")
    if not (math.isfinite(knee_db) and knee_db >= 0):
        raise ValueError(f"knee_db = {knee_db!r}: a finite width >= 0")
    if not math.isfinite(threshold_db):
        raise ValueError(f"threshold_db = {threshold_db!r}: a finite level")
    k = 1.0 - 1.0 / ratio
    d = np.asarray(level_db, dtype=np.float64) - threshold_db
    knee = k * (d + 0.5 * knee_db) ** 2 / (2.0 * knee_db) if knee_db > 0 else np.zeros_like(d)
    return np.where(2.0 * d < -knee_db, 0.0, np.where(2.0 * d <= knee_db, knee, k * d))


# ---- blind de-compression (BlindDynamicRangeOperator; csrc/drc_fit.hip): one parameter row per clip on the device
DRC_TABLE_COLUMNS = ("threshold_db", "slope", "makeup_db", "a_att", "a_rel", "1 - a_att", "1 - a_rel", "slope / (2 knee_db)")


def drc_table(threshold_db, slope, a_att, a_rel, makeup_db, knee_db, batch):
    """(batch, 8) np.float32 rows T, k, makeup, aA, aR, 1 - aA, 1 - aR, k / (2 W) for `drc_fwd_p` / `drc_bwd_p`.  Each of the five parameters
    is a scalar shared by the clips or holds one value per clip; each is rounded to fp32 first, and the derived entries are computed in
    float64 from those fp32 values and rounded once -- exactly as the host side of `drc_fwd` derives them, so a table of the parameters of a
    `drc_fwd` call gives its bits.  knee_db is the shared knee width W (k / (2 W) is 0 when W = 0)."""
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"batch = {batch!r}: at least one clip")
    knee = float(np.float32(knee_db))
    if not (math.isfinite(knee) and 0.0 <= knee <= 200.0):
        raise ValueError(f"knee_db = {knee_db!r}: a finite width in [0, 200]")
    cols = []
    for name, v in (("threshold_db", threshold_db), ("slope", slope), ("makeup_db", makeup_db), ("a_att", a_att), ("a_rel", a_rel)):
        v = np.asarray(v, dtype=np.float64).reshape(-1)
        if v.size not in (1, batch):
            raise ValueError(f"{name} holds {v.size} values: one, or one per clip of a batch of {batch}")
        cols.append(np.broadcast_to(v.astype(np.float32), (batch,)))
    T, k, m, aA, aR = cols
    out = np.empty((batch, 8), dtype=np.float32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4] = T, k, m, aA, aR
    out[:, 5] = (1.0 - aA.astype(np.float64)).astype(np.float32)
    out[:, 6] = (1.0 - aR.astype(np.float64)).astype(np.float32)
    out[:, 7] = (k.astype(np.float64) / (2.0 * knee)).astype(np.float32) if knee > 0 else 0.0
    return out


def drc_time_ms(a, sample_rate):
    """The time constant in milliseconds whose per-block coefficient is a: the inverse of `drc_coeffs` (0 for a = 1)."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(a >= 1.0, 0.0, -DRC_BLOCK / (float(sample_rate) * np.log1p(-np.minimum(a, 1.0))) * 1e3)


# ---- wow and flutter (TimeWarpOperator; csrc/warp.hip): a delay curve in samples, one knot per 64 samples, linear between the knots
WARP_BLOCK = 64
WARP_MAX_DELAY = 4096.0      # |d[j]|: a quarter of a second at 16 kHz; an fp32 delay of that size still resolves 2.4e-4 of a sample
WARP_MAX_STEP = 16.0         # |d[j+1] - d[j]|: the local speed within +-25 %, the read position strictly increasing


def warp_knots(length):
    """H + 1 = ceil(length / 64) + 1: the number of knots of the delay curve of a clip of `length` samples."""
    length = int(length)
    if length < 1:
        raise ValueError(f"length = {length!r}: at least one sample")
    return -(-length // WARP_BLOCK) + 1


def check_warp_curve(delay, name="delay"):
    """The contract of a delay curve ((K,) or (B, K) numpy fp32 knots in samples), refused by name: finite, |d[j]| <= 4096,
    |d[j+1] - d[j]| <= 16.  Returns the array."""
    d = np.asarray(delay)
    if d.dtype != np.float32 or d.ndim not in (1, 2) or d.shape[-1] < 2 or d.shape[0] < 1:
        raise ValueError(f"{name} has shape {d.shape} and dtype {d.dtype}: fp32 knots (K,) for every clip or (B, K), K = warp_knots(length) >= 2")
    if not np.isfinite(d).all():
        raise ValueError(f"{name}: every knot must be finite")
    worst = float(np.abs(d).max())
    if worst > WARP_MAX_DELAY:
        raise ValueError(f"{name}: |d[j]| reaches {worst!r} samples, the limit is {WARP_MAX_DELAY:g}")
    step = float(np.abs(np.diff(d.astype(np.float64), axis=-1)).max())
    if step > WARP_MAX_STEP:
        raise ValueError(f"{name}: |d[j+1] - d[j]| reaches {step!r} samples per block of {WARP_BLOCK}, the limit is {WARP_MAX_STEP:g} "
                         "(a local speed within +-25 %)")
    return d


# ---- blind wow and flutter (BlindTimeWarpOperator; csrc/warp_fit.hip): the curve lives on coarse knots, one every `knot_stride` fine knots
WARP_KNOT_STRIDES = (1, 2, 4, 8, 16, 32, 64)


def warp_coarse_knots(length, knot_stride):
    """P + 1 = ceil(H / knot_stride) + 1 coarse knots carry the curve of a clip of `length` samples (H = ceil(length / 64) blocks)."""
    if knot_stride not in WARP_KNOT_STRIDES or isinstance(knot_stride, bool):
        raise ValueError(f"knot_stride = {knot_stride!r}: a power of two from 1 to 64 (fine knots per coarse knot)")
    return -(-(warp_knots(length) - 1) // int(knot_stride)) + 1


def warp_expand(coarse, length, knot_stride):
    """Coarse knots (P + 1,) or (B, P + 1) -> the fine knots (H + 1,) or (B, H + 1) np.float32 that `warp_update` writes, in its arithmetic:
    d[S p + q] = fmaf(q / S, c[p+1] - c[p], c[p]), the difference rounded to fp32 first, q = 0 giving c[p] itself."""
    c = np.asarray(coarse, dtype=np.float32)
    K, n = warp_knots(length), warp_coarse_knots(length, knot_stride)
    if c.ndim not in (1, 2) or c.shape[-1] != n:
        raise ValueError(f"coarse has shape {c.shape}: ({n},) or (B, {n}) = warp_coarse_knots({length}, {knot_stride}) knots")
    j = np.arange(K)
    p, q = j // knot_stride, j % knot_stride
    c0 = c[..., p]
    c1 = c[..., np.minimum(p + 1, n - 1)]                     # never used where p = P: q = 0 there
    diff = (c1 - c0).astype(np.float32)
    fine = ((q / knot_stride) * diff.astype(np.float64) + c0.astype(np.float64)).astype(np.float32)
    return np.ascontiguousarray(np.where(q == 0, c0, fine))


def wow_curve(length, sample_rate, components=(), speed_percent=0.0):
    """The knots (warp_knots(length),) np.float32 of the delay curve, in samples, of a transport that runs `speed_percent` off speed and
    whose speed is modulated by `components` = ((rate_hz, depth_percent, phase_deg), ...) (phase optional) -- wow below about 6 Hz,
    flutter above:

        delta(t) = fs * [speed / 100 * t + sum_c depth_c / 100 * (sin(2 pi f_c t + p_c) - sin p_c) / (2 pi f_c)],    t = 64 j / fs

    the integral of the relative speed error, zero at t = 0; positive = reading ahead (the medium ran fast).  Computed in float64 and rounded
    once to fp32.  A result outside the contract of the curve (`check_warp_curve`) is refused by name."""
    K = warp_knots(length)
    sample_rate, speed_percent = float(sample_rate), float(speed_percent)
    if not (math.isfinite(sample_rate) and sample_rate > 0):
        raise ValueError(f"sample_rate = {sample_rate!r}: a positive finite rate")
    if not math.isfinite(speed_percent):
        raise ValueError(f"speed_percent = {speed_percent!r}: a finite percentage")
    t = np.arange(K, dtype=np.float64) * WARP_BLOCK / sample_rate
    delta = speed_percent / 100.0 * t
    for c in components:
        c = tuple(float(v) for v in c)
        if len(c) not in (2, 3) or not all(math.isfinite(v) for v in c) or c[0] <= 0:
            raise ValueError(f"components: {c!r} is not (rate_hz > 0, depth_percent[, phase_deg]), all finite")
        rate, depth, phase = c[0], c[1], math.radians(c[2]) if len(c) == 3 else 0.0
        w = 2.0 * math.pi * rate
        delta = delta + depth / 100.0 * (np.sin(w * t + phase) - math.sin(phase)) / w
    return check_warp_curve((sample_rate * delta).astype(np.float32), "wow_curve")


# ---- declicking (DeclickOperator, csrc/declick.hip)
CLICK_FRAME, CLICK_ORDER, CLICK_MAX_GUARD = 1024, 16, 64


def check_declick(threshold, sigma_floor, guard):
    """-> (threshold, sigma_floor, guard) as the kernels take them (fp32-rounded floats, an int), or a ValueError naming the argument."""
    try:
        t = float(np.float32(threshold))
    except (TypeError, ValueError):
        t = float("nan")
    if not (math.isfinite(t) and t > 0):
        raise ValueError(f"threshold = {threshold!r}: a finite number > 0 (the multiple of the robust scale above which a residual is a click)")
    try:
        f = float(np.float32(sigma_floor))
    except (TypeError, ValueError):
        f = float("nan")
    if not (math.isfinite(f) and f >= 0):
        raise ValueError(f"sigma_floor = {sigma_floor!r}: a finite number >= 0 (the smallest robust scale a frame is given)")
    if isinstance(guard, bool) or not isinstance(guard, (int, np.integer)) or not 0 <= int(guard) <= CLICK_MAX_GUARD:
        raise ValueError(f"guard = {guard!r}: an integer in 0 .. {CLICK_MAX_GUARD} (samples hidden on each side of a flagged one)")
    return t, f, int(guard)


def check_declick_fade(fade):
    if isinstance(fade, bool) or not isinstance(fade, (int, np.integer)) or not 0 <= int(fade) <= CLICK_MAX_GUARD:
        raise ValueError(f"fade = {fade!r}: an integer in 0 .. {CLICK_MAX_GUARD} (samples of cross-fade on each side of a masked run)")
    return int(fade)


def click_train(length, sample_rate, rate_hz, amplitude=(0.3, 0.6), max_width=3, seed=0, batch=1):
    """-> (batch, length) fp32 tensor of seeded sparse clicks for synthetic measurements: per clip round(rate_hz * length / sample_rate)
    clicks at uniform random positions, each with a random sign, an amplitude uniform in [lo, hi] and a width of 1 .. max_width samples
    (cut at the clip's end).  The same arguments give the same tensor; clip b depends on (seed, b) only."""
    lo, hi = (float(amplitude[0]), float(amplitude[1]))
    if not (isinstance(length, (int, np.integer)) and length >= 1 and isinstance(batch, (int, np.integer)) and batch >= 1):
        raise ValueError(f"length = {length!r}, batch = {batch!r}: positive integers")
    if not (math.isfinite(float(sample_rate)) and float(sample_rate) > 0 and math.isfinite(float(rate_hz)) and float(rate_hz) >= 0):
        raise ValueError(f"sample_rate = {sample_rate!r}, rate_hz = {rate_hz!r}: a positive rate and a click rate >= 0")
    if not (math.isfinite(lo) and math.isfinite(hi) and 0 <= lo <= hi):
        raise ValueError(f"amplitude = {amplitude!r}: (lo, hi) with 0 <= lo <= hi")
    if not (isinstance(max_width, (int, np.integer)) and max_width >= 1):
        raise ValueError(f"max_width = {max_width!r}: an integer >= 1")
    count = int(round(float(rate_hz) * length / float(sample_rate)))
    out = np.zeros((int(batch), int(length)), dtype=np.float32)
    for b in range(int(batch)):
        rng = np.random.default_rng([int(seed), b])
        pos = rng.integers(0, length, size=count)
        sign = rng.integers(0, 2, size=count) * 2 - 1
        amp = rng.uniform(lo, hi, size=count)
        width = rng.integers(1, int(max_width) + 1, size=count)
        for p, s, a, w in zip(pos, sign, amp, width):
            out[b, p:min(p + w, length)] = np.float32(s * a)
    import torch
    return torch.from_numpy(out)
