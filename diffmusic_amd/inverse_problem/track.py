"""Track mode: one recording of T samples restored as W overlapping model windows under ONE loss (extension; the reference restores
one window).

A track is one sample whose latent is the stack of its W windows.  Its waveform is `track = S(wav)`, wav the (W, >= L) vocoder
output, S the linear cross-fade below; the measurement operator, its transform and the loss act on the (1, T) track, and the gradient
reaches every window through S^T.  Both maps are one HIP launch (csrc/track.hip: `track_stitch_fwd` / `track_stitch_bwd`).

Layout, from (T, L, R), R the requested overlap in samples with 0 < R <= L // 2 and T >= L:
    W = 1 if T == L else 1 + ceil((T - L) / (L - R));   start[w] = (w * (T - L)) // (W - 1)
so consecutive windows overlap by at least R samples and every sample is covered -- by up to three windows (L = 6400, R = 1600,
T = 11300: starts 0, 2450, 4900).  Taper, the same for every window: u(i) = min(i + 0.5, L - 0.5 - i, R) / R.
    S:    track[n]   = sum_w (u(n - start[w]) / den[n]) * wav[w, n - start[w]],   den[n] = sum_w u(n - start[w])
    S^T:  dwav[w, i] = (u(i) / den[start[w] + i]) * dtrack[start[w] + i]  for i < L, zero for L <= i < full
A sample that one window covers is copied bit for bit; an overlap of exactly R samples is the linear cross-fade.

The windows are coupled in every step, so a track runs under a scheduler built with `per_clip_norm=False` (the loss is one scalar and
the update's norms go over all W windows), on one rank and one lane."""
import torch

from .. import ops
from .noise import step_sigma
from .operator import StyleGuidanceOperator

MAX_WINDOWS = 64          # csrc/track.hip: the window starts travel in the kernel arguments


def seconds_for_samples(samples, sample_rate):
    """The `audio_length_in_s` to give an operator that takes its length in seconds (`MusicInpaintingOperator` computes
    int(seconds * sample_rate)) so that it comes out at exactly `samples` samples: samples / sample_rate where that product rounds
    back, else the middle of the sample (a float quotient may land one ulp below the integer)."""
    seconds = samples / sample_rate
    if int(seconds * sample_rate) != int(samples):
        seconds = (samples + 0.5) / sample_rate
    assert int(seconds * sample_rate) == int(samples), (samples, sample_rate)
    return seconds


class TrackLayout:
    """Where the W windows of `window_len` samples sit in a track of `track_len` samples (rules in the module docstring)."""

    def __init__(self, track_len, window_len, overlap):
        T, L, R = int(track_len), int(window_len), int(overlap)
        if L < 2:
            raise ValueError(f"window_len = {window_len!r}: at least 2 samples")
        if T < L:
            raise ValueError(f"a track of {T} samples is shorter than one window of {L}: tracks shorter than a window are not supported")
        if R <= 0 or R > L // 2:
            raise ValueError(f"overlap = {overlap!r} samples: need 0 < overlap <= window_len // 2 = {L // 2}")
        self.track_len, self.window_len, self.overlap = T, L, R
        W = 1 if T == L else 1 + -((T - L) // -(L - R))
        self.num_windows = W
        self.starts = [0] if W == 1 else [(w * (T - L)) // (W - 1) for w in range(W)]

    def __repr__(self):
        return f"TrackLayout(track_len={self.track_len}, window_len={self.window_len}, overlap={self.overlap}) [{self.num_windows} windows]"

    def cut(self, track):
        """(T,) or (1, T) track -> its (W, L) windows, by plain slicing (e.g. `init_audio=layout.cut(y)` for a warm start)."""
        t = track.reshape(-1)
        if t.numel() != self.track_len:
            raise ValueError(f"track of {t.numel()} samples, layout of {self.track_len}")
        return torch.stack([t[s:s + self.window_len] for s in self.starts], dim=0)


class TrackOperator:
    """`inner` (a measurement operator built for the TRACK's length) applied to the stitched track of `layout`.

    forward / transform / inverse_transform / reset_cache / noiser are the inner operator's: they act on tracks.
    guidance(wav (W, full), length, measurement, space, **kw) -> ((1,) loss, (W, full) gradient): stitch, `inner.guidance` on the
    (1, T) track with every keyword passed through (`ir=`, `noise=`, `step=`, ...), then S^T."""

    # why the batch is ONE sample: a wrapper that carries this is refused per-clip norms, sharding and lanes (MixtureOperator has its own)
    one_sample = "a TrackOperator makes the batch one sample (the windows of a track under one loss)"

    def __init__(self, inner, layout):
        if isinstance(inner, TrackOperator):
            raise ValueError("TrackOperator around a TrackOperator: wrap the measurement operator itself")
        if isinstance(inner, StyleGuidanceOperator):
            raise ValueError("StyleGuidanceOperator cannot be the inner operator of a track: its CLAP tower is a 10-second model")
        if layout.num_windows > MAX_WINDOWS:
            raise ValueError(f"{layout.num_windows} windows: a track holds at most {MAX_WINDOWS}")
        self.inner, self.layout = inner, layout
        self.check_noise_stream()

    def check_noise_stream(self):
        noiser = self.noiser
        if step_sigma(noiser) > 0 and getattr(noiser, "stream", "global") == "clip":
            raise ValueError("track mode with measurement noise (sigma > 0) needs the global noise stream (GaussianNoise(sigma, "
                             "stream='global')): the per-clip stream keys one draw per clip, and a track is one sample made of all "
                             "its windows (teacher-forced `noise=` works too)")

    @property
    def noiser(self):
        return getattr(self.inner, "noiser", None)

    @property
    def cache_reference(self):
        return self.inner.cache_reference

    def dead_span(self, length):
        """None: the windows of a track overlap and are cross-faded into it, so a hole of the track is not one span shared by all
        windows (BaseOperator.dead_span)."""
        return None

    def forward(self, data, **kwargs):
        return self.inner.forward(data, **kwargs)

    def transform(self, *args, **kwargs):
        return self.inner.transform(*args, **kwargs)

    def inverse_transform(self, mel_spectrogram, vocoder):
        return self.inner.inverse_transform(mel_spectrogram, vocoder)

    def reset_cache(self):
        self.inner.reset_cache()

    def restart(self):
        restart = getattr(self.inner, "restart", None)
        if restart is not None:
            restart()

    def stitch(self, wav):
        """(W, >= L) fp32 windows on the GPU, any row stride -> the (1, T) track."""
        lay = self.layout
        if wav.dim() != 2 or wav.shape[0] != lay.num_windows or wav.shape[1] < lay.window_len:
            raise ValueError(f"wav has shape {tuple(wav.shape)}, expected ({lay.num_windows}, >= {lay.window_len}) for {lay!r}")
        return ops.hip.track_stitch_fwd(wav, lay.starts, lay.window_len, lay.overlap, lay.track_len)

    def stitch_transpose(self, dtrack, full):
        """(1, T) gradient w.r.t. the track -> (W, full) gradient w.r.t. the windows, zero past L."""
        lay = self.layout
        return ops.hip.track_stitch_bwd(dtrack.contiguous(), lay.starts, lay.window_len, lay.overlap, int(full))

    def guidance(self, wav, length, measurement, supervised_space, **kwargs):
        lay = self.layout
        if int(length) != lay.window_len:
            raise ValueError(f"original_waveform_length = {length}, but the track's windows hold {lay.window_len} samples")
        self.check_noise_stream()
        track = self.stitch(wav)
        loss, dtrack = self.inner.guidance(track, lay.track_len, measurement, supervised_space, **kwargs)
        return loss, self.stitch_transpose(dtrack, wav.shape[1])
