"""Source separation: K stems restored from their mixture y = sum_k g_k x_k under ONE loss (extension; the reference restores one signal
from one measurement).

The stems are the batch: each is a sample of the same prior under its own prompt embedding ("drums", "bass", ...), and the measurement
operator sees only their mix.  `mix = M(wav)`, wav the (K * G, >= L) vocoder output with stem-major rows (row k * G + w is stem k of group
w), M the gain-weighted sum over k; the inner operator, its transform and the loss act on the (G, L) mixture, and the gradient reaches
every stem through M^T.  Both maps are one HIP launch (csrc/mix.hip: `stem_mix_fwd` / `stem_mix_bwd`), feeding the inner operator's
existing kernels -- the mix is not fused into the STFT -> mel pair, whose per-frame gathers would read K rows about six times each.

`inner` is any measurement operator (G = 1: the mixture may also be clipped, reverberant, masked or noisy) or a `TrackOperator`
(G = layout.num_windows).  M is linear and the same for every window, so it commutes with the track stitch: a song longer than the model
window separates as `MixtureOperator(TrackOperator(inner, layout), K)`, the mixed windows going to `TrackOperator.guidance` as they are.

The stems are coupled in every step, so a mixture runs under a scheduler built with `per_clip_norm=False`, on one rank and one lane, and
its measurement noise comes from the global stream or a teacher-forced `noise=` (the rule of track mode).  One mixture per call."""
import math

import torch

from .. import ops
from .noise import step_sigma
from .operator import IdentityOperator, StyleGuidanceOperator
from .track import TrackOperator

MAX_STEMS = 16            # csrc/mix.hip: the gains travel in the kernel arguments


class MixtureOperator:
    """`inner` applied to the mix of `num_stems` stems with `gains` (None: all ones).

    forward(stems (K, L)) = inner.forward(mix); transform / inverse_transform / reset_cache / restart / noiser / cache_reference / dead_span
    are the inner operator's (a hole in the mixture hides the same samples of every stem).
    guidance(wav (K * G, full), length, measurement, space, **kw) -> ((1,) loss, (K * G, full) gradient): mix, `inner.guidance` on the
    (G, L) mixture with every keyword passed through, then M^T.
    project(stems, measurement): the opt-in output stage for a clean, plain mixture -- the minimum-norm correction after which the stems
    sum to the measurement (`stem_project`)."""

    one_sample = "a MixtureOperator makes the batch one sample (the stems of a mixture under one loss)"

    def __init__(self, inner, num_stems, gains=None):
        if isinstance(inner, MixtureOperator):
            raise ValueError("MixtureOperator around a MixtureOperator: wrap the measurement operator (or its TrackOperator) itself")
        if isinstance(inner, StyleGuidanceOperator):
            raise ValueError("StyleGuidanceOperator cannot be the inner operator of a mixture: style guidance has no measurement to "
                             "explain as a sum of stems")
        if isinstance(num_stems, bool) or not isinstance(num_stems, int) or not 1 <= num_stems <= MAX_STEMS:
            raise ValueError(f"num_stems = {num_stems!r}: an integer in 1 .. {MAX_STEMS}")
        if gains is not None:
            gains = [float(g) for g in (gains.tolist() if hasattr(gains, "tolist") else gains)]
            if len(gains) != num_stems:
                raise ValueError(f"{len(gains)} gains for {num_stems} stems: one gain per stem")
            if not all(math.isfinite(g) and math.isfinite(float(torch.tensor(g, dtype=torch.float32))) for g in gains):
                raise ValueError(f"gains = {gains!r}: finite fp32 values")
        self.inner, self.num_stems, self.gains = inner, num_stems, gains
        self.check_noise_stream()

    # ---- what the pipeline and the scheduler ask
    @property
    def track(self):
        """The inner TrackOperator, or None for a mixture of one window."""
        return self.inner if isinstance(self.inner, TrackOperator) else None

    @property
    def groups(self):
        return self.inner.layout.num_windows if isinstance(self.inner, TrackOperator) else 1

    @property
    def num_clips(self):
        """Rows of the batch: K stems times G windows."""
        return self.num_stems * self.groups

    def check_noise_stream(self):
        noiser = self.noiser
        if step_sigma(noiser) > 0 and getattr(noiser, "stream", "global") == "clip":
            raise ValueError("a mixture with measurement noise (sigma > 0) needs the global noise stream (GaussianNoise(sigma, "
                             "stream='global')): the per-clip stream keys one draw per clip, and a mixture is one sample made of all "
                             "its stems (teacher-forced `noise=` works too)")

    @property
    def noiser(self):
        return getattr(self.inner, "noiser", None)

    @property
    def cache_reference(self):
        return self.inner.cache_reference

    def dead_span(self, length):
        span = getattr(self.inner, "dead_span", None)
        return span(length) if span is not None else None

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

    # ---- M and M^T
    def mix(self, wav, length=None, groups=None):
        """(K * G, >= length) fp32 stems on the GPU, stem-major rows, any row stride -> the (G, length) mixtures."""
        G = self.groups if groups is None else int(groups)
        length = wav.shape[1] if length is None else int(length)
        if wav.dim() != 2 or wav.shape[0] != self.num_stems * G or wav.shape[1] < length:
            raise ValueError(f"wav has shape {tuple(wav.shape)}, expected ({self.num_stems * G}, >= {length}): {self.num_stems} stems of "
                             f"{G} window(s)")
        return ops.hip.stem_mix_fwd(wav, self.gains, self.num_stems, G, length)

    def mix_transpose(self, dmix, full):
        """(G, L) gradient w.r.t. the mixtures -> (K * G, full) gradient w.r.t. the stems, zero past L."""
        return ops.hip.stem_mix_bwd(dmix.contiguous(), self.gains, self.num_stems, int(full))

    def forward(self, data, **kwargs):
        """data (K, L): the stems of ONE signal (whole tracks when the inner operator is a track's) -> the measurement of their mix."""
        if not data.is_cuda:
            raise RuntimeError("diffmusic_amd operators run on the GPU only (HIP library); move the tensor to cuda")
        data = data.to(torch.float32)
        if data.dim() == 2 and data.stride(1) != 1:
            data = data.contiguous()
        return self.inner.forward(self.mix(data, groups=1), **kwargs)

    def guidance(self, wav, length, measurement, supervised_space, **kwargs):
        self.check_noise_stream()
        mix = self.mix(wav, length)
        loss, dmix = self.inner.guidance(mix, length, measurement, supervised_space, **kwargs)
        return loss, self.mix_transpose(dmix, wav.shape[1])

    # ---- output stages
    def stitch_stems(self, wav):
        """Mixture of a track: the (K * W, >= L) windows -> the (K, T) stems, each stitched from its W contiguous rows."""
        track, W = self.track, self.groups
        return torch.cat([track.stitch(wav[k * W:(k + 1) * W]) for k in range(self.num_stems)], dim=0)

    def project(self, stems, measurement):
        """-> (K, L), L the measurement's length: p_k = x_k + c_k (y - mix(x)), c_k = g_k / sum_j g_j^2, the smallest change of the
        restored stems after which they sum to the mixture.  Opt-in; only where the measurement IS the mixture: an IdentityOperator
        inside (of a track too: then on the stitched (K, T) stems) and no measurement noise."""
        inner = self.inner.inner if isinstance(self.inner, TrackOperator) else self.inner
        if not isinstance(inner, IdentityOperator):
            raise ValueError(f"project: the measurement of {type(inner).__name__} is not the mixture itself; only a plain mixture "
                             "(IdentityOperator inside) can be projected onto")
        if step_sigma(self.noiser) > 0:
            raise ValueError("project: the measurement carries additive noise (sigma > 0), so the stems need not sum to it")
        y = torch.as_tensor(measurement)
        if not y.is_cuda:
            raise RuntimeError("diffmusic_amd operators run on the GPU only (HIP library); move the tensor to cuda")
        y = y.to(torch.float32).reshape(1, -1).contiguous()
        x = torch.as_tensor(stems).to(device=y.device, dtype=torch.float32)
        if x.dim() != 2 or x.shape[0] != self.num_stems or x.shape[1] < y.shape[1]:
            raise ValueError(f"project: stems {tuple(x.shape)} do not cover the mixture {tuple(y.shape)} with {self.num_stems} rows")
        if x.stride(1) != 1:
            x = x.contiguous()
        return ops.hip.stem_project(x, y, self.gains, y.shape[1])
