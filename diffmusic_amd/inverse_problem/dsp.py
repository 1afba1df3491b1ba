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
