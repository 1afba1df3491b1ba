"""Measurement operators A(.) with the reference's BaseOperator protocol
(diffmusic/inverse_problem/operator.py:6-14): forward / transform / inverse_transform, same
constructor signatures as run.py:164-212 uses.  All arithmetic runs in the HIP library
(csrc/mel.hip) on the input tensor's device -- the reference's hard-coded .to("cuda")
(operator.py:33,83,149,191,226) is not reproduced.

Extension used by the guided schedulers (no torch.autograd on the hot path):
`guidance(wav, L, measurement, supervised_space)` returns the per-clip loss ||y - A(wav)|| (in the
chosen space) and its gradient with respect to the vocoder output, computed by hand-written
backward kernels (the reference gets the same quantity from torch.autograd.grad,
scheduling_dps.py:202-212).

An operator defines A once: `apply(x, length, **kw) -> (y, adjoint)` gives y = A(x[:, :length]) without measurement noise and a
closure `adjoint(dy, full)`, the transpose of dA/dx at x.  The closure captures whatever the transpose needs (the input of a clip, the
input length of a FIR, the impulse response of that call); nothing about one call is kept on the operator.  `forward` is `apply` plus
the noiser, and `BaseOperator.guidance` is the one driver of the guided step: `apply`, the step's noise, the loss in the supervised
space, `adjoint`.  In mel space `_MelOperator` first asks `_on_load` whether A can ride inside the fused STFT-mel kernels.
The operators that fit parameters of their own along the way (`after_cotangent`) live in blind.py, which imports this module.

Measurement noise inside the step: the reference's `forward` ends in `self.noiser(...)` and its schedulers call it on the
predicted audio in every step, so with sigma > 0 the loss is taken on A(wav) + sigma * z.  `guidance(..., noise=None, step=None,
generator=None)` does the same when the operator's noiser has `additive_sigma > 0`: z is `noise` when given (a standard-normal
tensor shaped like A(wav), for teacher forcing) and otherwise a device-side draw of the noiser (`GaussianNoise.draw`, keyed by
`step` / `generator` on the clip stream).  The noise is additive and independent of wav: the gradient has no extra term.  With
sigma == 0, no noiser, or a noiser without an additive part (Poisson) nothing is drawn or launched."""
import ctypes as C
import math
import numpy as np
import torch

from .. import _lib as L
from .. import ops
from . import dsp
from .noise import step_sigma

_NEG, _POS = -3.0e38, 3.0e38


class SpectralFrontend:
    """dmx_audio handle: STFT(n_fft, hop) + mel filterbank, forward and hand-written backward.
    Equivalent of torchaudio MelSpectrogram(+AmplitudeToDB) / MelScale / torch.stft in the reference."""

    def __init__(self, sample_rate=16000, n_fft=1024, hop_length=160, n_mels=64, window="hann", fb=None):
        """fb: optional (n_fft/2+1, n_mels) filterbank replacing the default torchaudio-style HTK one (CLAP's slaney bank)."""
        self.n_fft, self.hop, self.n_mels, self.bins = n_fft, hop_length, n_mels, n_fft // 2 + 1
        if fb is None:
            fb = dsp.melscale_fbanks(self.bins, 0.0, float(sample_rate // 2), n_mels, sample_rate)
        fb = np.ascontiguousarray(np.asarray(fb, dtype=np.float32))
        assert fb.shape == (self.bins, n_mels), fb.shape
        self._h = C.c_void_p(L.lib().dmx_audio_create(n_fft, hop_length, n_mels, 1 if window == "hann" else 0,
                                                       fb.ctypes.data_as(C.c_void_p)))
        if not self._h:
            L.check(-1, "dmx_audio_create")
        self._state = None

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                L.lib().dmx_audio_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def frames(self, length):
        return 1 + length // self.hop

    def _get_state(self, B, length, device):
        n = L.lib().dmx_audio_state_bytes(self._h, B, length)
        if self._state is None or self._state.numel() < n or self._state.device != device:
            self._state = torch.empty(n, dtype=torch.uint8, device=device)
        return self._state

    def transform_fwd(self, wav, length, power2=True, to_db=True, lo=_NEG, hi=_POS, out=None):
        """wav: fp32 cuda (B, >=length) with arbitrary row stride -> (B, frames, n_mels) fp32."""
        assert wav.dtype == torch.float32 and wav.is_cuda and wav.stride(1) == 1
        B = wav.shape[0]
        st = self._get_state(B, length, wav.device)
        self._last = (B, length, power2, to_db, lo, hi)
        return ops.hip.logmel_fwd(self._h.value, wav, st, int(length), bool(power2), bool(to_db), float(lo), float(hi), out=out)

    def transform_bwd(self, dmel, dwav=None):
        """dwav: caller-owned (B, >= length) gradient with any row stride."""
        B, length, power2, to_db, lo, hi = self._last
        return ops.hip.logmel_bwd(self._h.value, dmel.contiguous(), self._state, int(length), bool(power2), bool(to_db), float(lo), float(hi),
                                  dwav=dwav)

    def fused(self, length):
        """True when the fused STFT -> mel kernels (csrc/stft_mel.hip: n_fft = 1024) cover this handle and clip length."""
        return bool(L.lib().dmx_audio_is_fused(self._h, int(length)))

    def guidance(self, wav, length, ref, mask=None, power2=True, to_db=True, lo=_NEG, hi=_POS, gscale=1.0, noise=None, noise_mag=None,
                 sigma=0.0, thr=None):
        """Fused guidance pair: loss[b] = ||ref[b] - transform(wav[b, :length] * mask)||_2 and dwav = gscale * dloss/dwav, (B, wav.shape[1])
        with zeros past `length` -- one forward and one backward launch, no spectrum in HBM (op `mel_guidance`).
        noise (B, >= length) / noise_mag (B, bins, frames; power2 False): standard-normal draws entering as wav * mask + sigma * noise,
        resp. |STFT| + sigma * noise_mag, inside both kernels.
        thr (B) fp32: per-clip hard-clip thresholds, y = clip(wav * mask, thr) + sigma * noise inside both kernels."""
        assert wav.dtype == torch.float32 and wav.is_cuda and wav.stride(1) == 1 and ref.dtype == torch.float32 and ref.is_contiguous()
        B, full = wav.shape
        st = self._get_state(B, length, wav.device)
        return ops.hip.mel_guidance(self._h.value, wav, mask, ref, st, int(length), int(full), bool(power2), bool(to_db), float(lo),
                                    float(hi), float(gscale), noise, noise_mag, float(sigma), thr)

    def stft_mag(self, wav, length):
        B = wav.shape[0]
        st = self._get_state(B, length, wav.device)
        return ops.hip.stft_mag_fwd(self._h.value, wav, st, int(length))

    def stft_mag_bwd(self, dmag, length, dwav):
        """dmag (B, bins, frames) w.r.t. the magnitude of the last stft_mag call -> dwav (B, >=length) (overwritten)."""
        return ops.hip.stft_mag_bwd(self._h.value, dmag, self._state, int(length), dwav.shape[1], dwav=dwav)

    def melscale(self, mag, lo=_NEG, hi=_POS):
        return ops.hip.melscale_fwd(self._h.value, mag.contiguous(), float(lo), float(hi))


class ModelMelFrontend:
    """Waveform -> mel in the domain the VAE / vocoder work in, for warm-started sampling (`init_audio`): STFT magnitudes (hann, centred,
    reflect-padded) through a slaney-normalised mel bank, then the natural log with a floor.  The log is NOT taken here: `__call__`
    returns the linear magnitudes and the encoder's input stage applies ln(max(x, log_floor)) on load (VaeEncoderEngine.encode,
    `log_floor=`).  The defaults (n_fft 1024, hop 160, 64 bins, 0-8000 Hz, floor 1e-5) are the AudioLDM / MusicLDM training front end
    as recalled -- that code is third-party and was not available to check against, so every one of them is a constructor argument."""

    def __init__(self, sample_rate=16000, n_fft=1024, hop_length=160, n_mels=64, f_min=0.0, f_max=8000.0, log_floor=1e-5):
        from transformers.audio_utils import mel_filter_bank
        self.fb = mel_filter_bank(num_frequency_bins=n_fft // 2 + 1, num_mel_filters=n_mels, min_frequency=float(f_min),
                                  max_frequency=float(f_max), sampling_rate=sample_rate, norm="slaney", mel_scale="slaney")
        self.frontend = SpectralFrontend(sample_rate, n_fft, hop_length, n_mels, "hann", fb=self.fb)
        self.log_floor = float(log_floor)

    def __call__(self, wav, length, frames):
        """wav (B, >= length) fp32 cuda -> (B, frames, n_mels) fp32 linear mel magnitudes: the clip's 1 + length // hop frames cropped, or
        padded with the floor value (ln gives the floor's log there), to `frames`."""
        mel = self.frontend.transform_fwd(wav, int(length), power2=False, to_db=False)
        have = mel.shape[1]
        if have >= frames:
            return mel[:, :frames].contiguous()
        return torch.nn.functional.pad(mel, (0, 0, 0, frames - have), value=self.log_floor).contiguous()


def l2_loss(ref, pred, want_grad=True, gscale=1.0):
    """per-clip ||ref - pred||_2 over all trailing dims; ref may have batch 1 (broadcast), pred is contiguous."""
    ref = ref.contiguous()
    assert ref[0].numel() == pred[0].numel() and pred.is_contiguous(), (ref.shape, pred.shape, pred.stride())
    return ops.hip.l2norm(ref, pred, float(gscale), want_grad=want_grad)


def _as_f32_cuda(x):
    if not x.is_cuda:
        raise RuntimeError("diffmusic_amd operators run on the GPU only (HIP library); move the tensor to cuda")
    return x.to(torch.float32)


def _flat_rows(m):
    return m.reshape(m.shape[0], -1).contiguous()


class BaseOperator:
    """forward(data) = noiser(A(data)); transform(x) = supervised-space map; inverse_transform(mel, vocoder)."""
    noiser = None

    def transform(self, data, *args, **kwargs):
        raise NotImplementedError

    def inverse_transform(self, mel_spectrogram, vocoder):      # operator.py:38-42 (six identical copies)
        if mel_spectrogram.dim() == 4:
            mel_spectrogram = mel_spectrogram.squeeze(1)
        return vocoder(mel_spectrogram)

    def apply(self, x, length, **kw):
        """x (B, >= length) fp32 on the GPU, any row stride -> (y, adjoint).
        y = A(x[:, :length]), contiguous fp32, WITHOUT measurement noise.
        adjoint(dy, full) -> (B, full) fp32: the transpose of dA/dx at x applied to dy, zeros past `length`."""
        raise NotImplementedError

    def _measure(self, y):
        return self.noiser(y) if self.noiser is not None else y

    def forward(self, data, **kwargs):
        return self._measure(self.apply(_as_f32_cuda(data), data.shape[-1], **kwargs)[0])

    # ---- guided-step extension -------------------------------------------------------------
    _ref_cache = None
    cache_reference = True     # False: recompute transform(measurement) every step, as the reference does (operator.py:205-206 call site)

    def reset_cache(self):
        """Forget the cached `transform(measurement)` and restart the noiser's step stream; called at the start of every trajectory
        (set_timesteps / __call__)."""
        self._ref_cache = None
        reset = getattr(self.noiser, "reset", None)
        if reset is not None:
            reset()

    def _ref(self, measurement, space, fn):
        """`transform(y)` is constant over a trajectory: computed once per measurement TENSOR and supervised space.  A cache
        entry holds the tensor itself (identity comparison + version counter), which also keeps its storage alive, so a later
        measurement can never be handed the same address by the caching allocator and hit a stale entry.  A few entries are kept
        (most recent first): the clip lanes of one call (pipelines/lanes.py) alternate between their measurement tensors."""
        if not self.cache_reference:
            return fn(_as_f32_cuda(measurement))
        cache = self._ref_cache
        if cache is None:
            cache = self._ref_cache = []
        for c in cache:
            if c[0] is measurement and c[1] == measurement._version and c[2] == space:
                return c[3]
        cache.insert(0, (measurement, measurement._version, space, fn(_as_f32_cuda(measurement))))
        del cache[4:]
        return cache[0][3]

    def guidance(self, wav, length, measurement, supervised_space, noise=None, step=None, generator=None, **apply_kw):
        """-> (loss (B), dwav (B, wav.shape[1])): ||transform(measurement) - transform(A(wav[:, :length]) + sigma * z)||_2 per clip and
        its gradient; `apply_kw` goes to `apply` (`ir=` of the dereverberation)."""
        if supervised_space == "mel_spectrogram":
            return self._mel_guidance(wav, length, measurement, noise, step, generator, **apply_kw)
        if supervised_space != "wav_form":
            raise ValueError("supervised_space should be either 'wav_form' or 'mel_spectrogram")
        y, adjoint = self._noisy_apply(wav, length, noise, step, generator, **apply_kw)
        loss, dy = l2_loss(self._ref(measurement, "wav_form", _flat_rows), y.reshape(y.shape[0], -1))
        return loss, self._pull_back(adjoint, wav, length, dy.reshape(y.shape), apply_kw)

    def _pull_back(self, adjoint, x, length, dy, apply_kw):
        """dwav = adjoint(dy), then the operator's look at the step's cotangent: the gradient is the one of the operator `apply` used."""
        dwav = adjoint(dy, x.shape[1])
        self.after_cotangent(x, length, dy, **apply_kw)
        return dwav

    def after_cotangent(self, x, length, dy, **apply_kw):
        """Called by `guidance` once per step with dy = d loss / d y at y = A(x[:, :length]) (+ noise), y materialised by `apply`, after
        the gradient w.r.t. x has been taken: an operator with parameters of its own updates them here (blind.py, `_FittedOperator`).
        Not called where A rides inside the fused mel kernels (`_on_load`): no dy exists there.  No-op by default."""

    def restart(self):
        """The pipeline restarts the current trajectory from fresh latents (NaN-retry): state that a trajectory builds up goes back to
        its start (`_FittedOperator`: the estimate, its moments and k).  Nothing by default -- the cached reference and the noiser's stream
        are kept, as they always were."""

    # (who, what) where the operator keeps state indexed by batch position -- per-clip parameters, given or fitted -- else None: the
    # pipelines then refuse clip lanes and sharding with "<who> cannot ...: its <what> are indexed by batch position"
    positional_state = None

    def _mel_guidance(self, wav, length, measurement, noise, step, generator, **apply_kw):
        raise NotImplementedError

    def _noisy_apply(self, wav, length, noise, step, generator, **apply_kw):
        """`apply` with this step's measurement noise on the materialised y; the noise is additive, so the transpose is unchanged."""
        y, adjoint = self.apply(wav, length, **apply_kw)
        z, sigma = self._step_noise(y.shape, y.device, noise, step, generator)
        if z is not None:
            y = ops.hip.noise_add(y, z, sigma)
        return y, adjoint

    def dead_span(self, length):
        """The longest run of samples [s0, s1) of a waveform of `length` samples on which, for EVERY clip of the batch, A(wav) does not
        depend on wav and the gradient `guidance` returns is identically zero -- or None.  The guided step hands it to the vocoder,
        which then skips the rows that reach only those samples (HifiGanEngine.forward, `dead=`).  Only an operator that can prove
        it overrides this; measurement noise (sigma > 0) is added after A and changes nothing."""
        return None

    def _step_noise(self, shape, device, noise, step, generator):
        """-> (z, sigma): the standard-normal tensor of shape `shape` = A(wav).shape that this step adds as sigma * z, or (None, 0.0).
        Decided by the noiser's explicit `additive_sigma` (noise.py); `noise` given = teacher forcing, else the noiser draws."""
        sigma = step_sigma(self.noiser)
        if sigma <= 0.0:
            return None, 0.0
        if noise is None:
            return self.noiser.draw(tuple(shape), device, step=step, generator=generator), sigma
        if tuple(noise.shape) != tuple(shape):
            raise ValueError(f"noise must be shaped like A(x) = {tuple(shape)}, got {tuple(noise.shape)}")
        return _as_f32_cuda(noise).contiguous(), sigma


class _MelOperator(BaseOperator):
    """Shared mel plumbing: transform = wav2mel (dB) between the `clamp` bounds; returns (B, n_mels, T)."""
    clamp = (-80.0, 80.0)

    def _init_mel(self, sample_rate=16000, lazy=False):
        """lazy: the front end (GPU tables) is made on first use, so the operator can be built without a GPU."""
        self._mel_rate, self._frontend = sample_rate, None
        if not lazy:
            self.frontend

    @property
    def frontend(self):
        if self._frontend is None:
            self._frontend = SpectralFrontend(self._mel_rate, 1024, 160, 64, "hann")
        return self._frontend

    def _mel(self, audio, length=None):
        audio = _as_f32_cuda(audio)
        return self.frontend.transform_fwd(audio, length or audio.shape[-1], True, True, *self.clamp)

    def transform(self, audio):
        return self._mel(audio).transpose(1, 2)             # torchaudio layout (B, n_mels, frames)

    def _on_load(self, wav, length):
        """The extra operands (`mask=`, `thr=` of SpectralFrontend.guidance) with which the fused mel kernels apply A themselves while they
        load wav[:, :length], or None: A has to be materialised by `apply`."""
        return None

    def _mel_ref(self, measurement):
        return self._ref(measurement, "mel_spectrogram", lambda m: self._mel(m.reshape(m.shape[0], -1)).clone())

    def _mel_guidance(self, wav, length, measurement, noise, step, generator, **apply_kw):
        lo, hi = self.clamp
        operands = self._on_load(wav, length)
        if operands is not None and self.frontend.fused(length):
            # A, noise, STFT, mel, dB, L2 and the whole backward in two launches; y = A(wav) is never materialised
            ref = self._mel_ref(measurement)
            z, sigma = self._step_noise((wav.shape[0], length), wav.device, noise, step, generator)
            return self.frontend.guidance(wav, length, ref, lo=lo, hi=hi, noise=z, sigma=sigma, **operands)
        y, adjoint = self._noisy_apply(wav, length, noise, step, generator, **apply_kw)      # y (B, L') contiguous fp32
        ref = self._mel_ref(measurement)
        if self.frontend.fused(y.shape[1]):
            loss, dy = self.frontend.guidance(y, y.shape[1], ref, lo=lo, hi=hi)
        else:
            loss, dmel = l2_loss(ref, self._mel(y))
            dy = self.frontend.transform_bwd(dmel)
        return loss, self._pull_back(adjoint, wav, length, dy, apply_kw)


def longest_zero_run(mask):
    """(s0, s1) of the longest run of exact zeros in a 1-D host mask (the first of equally long ones), or None without a zero."""
    z = np.concatenate(([0], (np.asarray(mask, dtype=np.float32).reshape(-1) == 0).astype(np.int8), [0]))
    edges = np.flatnonzero(np.diff(z))                       # run starts at even positions, ends (exclusive) at odd ones
    if edges.size == 0:
        return None
    starts, ends = edges[0::2], edges[1::2]
    i = int(np.argmax(ends - starts))
    return int(starts[i]), int(ends[i])


def _masked(x, length, mask):
    """-> (x[:, :length] * mask, adjoint) for a (1, length) mask on x's device, or None for the plain crop: a per-sample mask is its own
    transpose, and the transpose of the crop is the zero-pad."""
    def adjoint(dy, full):
        return ops.hip.mask_mul(dy, mask, dy.shape[1], int(full))
    return ops.hip.mask_mul(x, mask, int(length), int(length)), adjoint


class IdentityOperator(_MelOperator):                     # operator.py:17-45
    def __init__(self, sample_rate):
        self._init_mel(sample_rate)

    def forward(self, data, **kwargs):
        return data

    def apply(self, x, length, **kw):
        return _masked(x, length, None)

    def _on_load(self, wav, length):
        return {}


class MusicInpaintingOperator(_MelOperator):              # operator.py:48-133
    clamp = (_NEG, _POS)                                    # transform = wav2mel without clamp (operator.py:123-124)

    def __init__(self, audio_length_in_s, sample_rate, mask_type, start_inpainting_s, end_inpainting_s, mask_percentage,
                 mask_duration_s, interval_s, noiser=None):
        self.audio_length_in_s, self.sample_rate, self.mask_type = audio_length_in_s, sample_rate, mask_type
        self.start_inpainting_s, self.end_inpainting_s = start_inpainting_s, end_inpainting_s
        self.mask_percentage, self.interval_s, self.mask_duration_s = mask_percentage, interval_s, mask_duration_s
        self.mask = self.generate_mask()
        self._init_mel(sample_rate)
        self.noiser = noiser
        self._mask_dev = None

    def generate_mask(self):                                # operator.py:87-121 (host, once)
        n = int(self.audio_length_in_s * self.sample_rate)
        mask = torch.ones([1, n])
        sr = self.sample_rate
        if self.mask_type == "box":
            if self.start_inpainting_s is not None and self.end_inpainting_s is not None:
                mask[:, int(self.start_inpainting_s * sr): int(self.end_inpainting_s * sr)] = 0.
        elif self.mask_type == "random":
            dur = int(self.mask_duration_s * sr)
            count = max(1, int(self.mask_percentage * n) // dur)
            for _ in range(count):
                start = int(torch.randint(0, mask.shape[1] - dur, (1,)))
                mask[:, start:start + dur] = 0.
        elif self.mask_type == "periodic":
            interval, dur = int(self.interval_s * sr), int(self.mask_duration_s * sr)
            for start in range(0, mask.shape[1], interval):
                mask[:, start:min(start + dur, mask.shape[1])] = 0.
        return mask

    def dead_span(self, length):
        """The longest run of zeros of the mask (one (1, n) mask for all clips, fixed at construction): found on the host once and kept
        with the mask it was found in."""
        if length != self.mask.shape[1]:
            return None
        cached = getattr(self, "_dead_span", None)
        if cached is None or cached[0] is not self.mask or cached[1] != self.mask._version:
            cached = self._dead_span = (self.mask, self.mask._version, longest_zero_run(self.mask[0]))
        return cached[2]

    def _mask_on(self, device):
        if self._mask_dev is None or self._mask_dev.device != device:
            self._mask_dev = self.mask.to(device=device, dtype=torch.float32).contiguous()
        return self._mask_dev

    def _mask_for(self, device, length):
        if length != self.mask.shape[1]:
            raise ValueError(f"mask length {self.mask.shape[1]} != waveform length {length}")
        return self._mask_on(device)

    def apply(self, x, length, **kw):
        return _masked(x, length, self._mask_for(x.device, length))

    def _on_load(self, wav, length):
        return dict(mask=self._mask_for(wav.device, length))


class DeclippingOperator(_MelOperator):
    """Hard clipping (extension; the reference has no nonlinear operator): A(x)[b, s] = min(max(x[b, s], -c[b]), c[b]) with one threshold
    c[b] > 0 per clip, forward = noiser(A(x)), transform = clamp(wav2mel, -80, 80) like the IdentityOperator's.

    threshold: a positive float (every clip), a sequence or a (B,) tensor (one per clip; the batch of `forward` / `guidance` must then be
    B -- inside a TrackOperator that is the one track).  dA/dx = 1 on -c <= x <= c (torch.clamp's rule at equality), 0 outside: a restored
    sample beyond the threshold on the right side costs nothing, and the loss pulls only through the unclipped positions.  A NaN sample
    stays NaN.  In mel space with fused kernels the clip happens on load inside the guidance pair (csrc/stft_mel.hip); elsewhere through
    `clip_fwd` / `clip_bwd` (csrc/waveshape.hip).  `project` is the optional output stage.

    The front end and the device copy of the thresholds are made on first use, so the operator can be built without a GPU."""

    def __init__(self, sample_rate, threshold, noiser=None):
        thr = torch.as_tensor(threshold, dtype=torch.float32).detach().cpu().reshape(-1)
        if thr.numel() < 1 or not bool(torch.isfinite(thr).all()) or not bool((thr > 0).all()):
            raise ValueError(f"threshold = {threshold!r}: positive finite value(s), one for all clips or one per clip")
        self.sample_rate, self.noiser = sample_rate, noiser
        self.per_clip = torch.as_tensor(threshold).dim() > 0      # a scalar broadcasts over any batch
        self.threshold = thr.clone()                          # host copy: (1,) broadcast over the batch, or (B,)
        self._thr_dev = None
        self._init_mel(sample_rate, lazy=True)

    def _check_batch(self, batch):
        n = self.threshold.numel()
        if self.per_clip and n != batch:
            raise ValueError(f"DeclippingOperator holds {n} per-clip threshold(s), the batch has {batch} clip(s)")

    def thresholds(self, batch, device):
        """The (batch,) fp32 thresholds on `device` (one tensor, kept)."""
        self._check_batch(batch)
        t = self._thr_dev
        if t is None or t.device != device or t.numel() != batch:
            t = self._thr_dev = self.threshold.to(device).expand(batch).contiguous()
        return t

    def forward(self, data, **kwargs):
        self._check_batch(data.shape[0])                      # before the tensor has to be on the GPU
        return super().forward(data, **kwargs)

    def apply(self, x, length, **kw):
        thr = self.thresholds(x.shape[0], x.device)

        def adjoint(dy, full):                                # the Jacobian of a nonlinear A is taken at x
            return ops.hip.clip_bwd(dy.contiguous(), x, thr, int(full))
        return ops.hip.clip_fwd(x, thr, int(length)), adjoint

    def _on_load(self, wav, length):
        return dict(thr=self.thresholds(wav.shape[0], wav.device))

    def project(self, wav, measurement):
        """The conventional output stage of declipping -> (B, L), L the measurement's length: reliable samples (|y| < c) are the
        measurement's, clipped ones are the restored sample pushed to the clipped side (max(x, c) for y >= c, min(x, -c) for y <= -c).
        Opt-in; refused with measurement noise, under which no sample of y is reliable."""
        if step_sigma(self.noiser) > 0:
            raise ValueError("project: the measurement carries additive noise (sigma > 0), so none of its samples is reliable")
        y = _as_f32_cuda(measurement)
        y = y.reshape(y.shape[0], -1)
        wav = _as_f32_cuda(torch.as_tensor(wav).to(y.device))
        wav = wav.reshape(wav.shape[0], -1)
        if wav.shape[0] != y.shape[0] or wav.shape[1] < y.shape[1]:
            raise ValueError(f"project: restored audio {tuple(wav.shape)} does not cover the measurement {tuple(y.shape)}")
        if wav.stride(1) != 1:
            wav = wav.contiguous()
        return ops.hip.declip_project(wav, y.contiguous(), self.thresholds(y.shape[0], y.device), y.shape[1])


class PhaseRetrievalOperator(BaseOperator):               # operator.py:136-171
    def __init__(self, n_fft=1024, hop_length=160, win_length=1024, noiser=None):
        assert win_length == n_fft
        self.n_fft, self.hop_length, self.win_length = n_fft, hop_length, win_length
        self.frontend = SpectralFrontend(16000, n_fft, hop_length, 64, "rect")   # torch.stft(window=None)
        self.noiser = noiser

    def transform(self, magnitude):                        # clamp(MelScale(mag), -80, 80) -> (B, n_mels, T)
        return self.frontend.melscale(_as_f32_cuda(magnitude), -80.0, 80.0).transpose(1, 2)

    def apply(self, x, length, **kw):
        """y = |STFT(x)| (B, bins, frames): the `wav_form` loss is taken on the raw magnitudes (scheduling_dps.py:199-201).  The transpose
        divides by the clean |X| that the front end's state keeps until its next transform."""
        def adjoint(dmag, full):
            dwav = torch.zeros(x.shape[0], full, dtype=torch.float32, device=x.device)
            self.frontend.stft_mag_bwd(dmag, length, dwav)
            return dwav
        return self.frontend.stft_mag(x, length), adjoint

    def _mel_guidance(self, wav, length, measurement, noise, step, generator, **apply_kw):
        bins_frames = (wav.shape[0], self.frontend.bins, self.frontend.frames(length))
        ref = self._ref(measurement, "mel_spectrogram", lambda m: self.frontend.melscale(m, -80.0, 80.0))
        z, sigma = self._step_noise(bins_frames, wav.device, noise, step, generator)
        if self.frontend.fused(length):
            return self.frontend.guidance(wav, length, ref, None, False, False, -80.0, 80.0, noise_mag=z, sigma=sigma)
        if z is not None:
            raise NotImplementedError("phase retrieval with measurement noise in mel space needs the fused kernels (n_fft = 1024, clips of "
                                      ">= 2048 samples): the dense-DFT path has no entry for the magnitude-domain noise")
        pred = self.frontend.transform_fwd(wav, length, False, False, -80.0, 80.0)   # |STFT| -> MelScale -> clamp
        loss, dmel = l2_loss(ref, pred)
        dwav = torch.zeros(wav.shape[0], wav.shape[1], dtype=torch.float32, device=wav.device)
        self.frontend.transform_bwd(dmel, dwav)
        return loss, dwav


def _fir_fwd(x, x_len, h, out_len, orig, new, off):
    return ops.hip.resample_fwd(x, h, int(x_len), int(out_len), int(orig), int(new), int(off))


def _fir_bwd(dy, h, h_rev, in_len, full_len, orig, new, off):
    """gradient w.r.t. the first in_len samples of a (B, full_len) input; the tail gets zero."""
    return ops.hip.resample_bwd(dy.contiguous(), h, h_rev, int(in_len), int(full_len), int(orig), int(new), int(off))


class SuperResolutionOperator(_MelOperator):              # operator.py:174-205
    """forward = torchaudio Resample(sample_rate -> sample_rate // scale) (sinc_interp_hann, width 6, rolloff 0.99);
    transform = clamp(wav2mel) applied to the low-rate signal with the 16 kHz mel parameters."""

    def __init__(self, sample_rate, scale=10, noiser=None):
        self.orig_freq, self.new_freq = sample_rate, sample_rate // scale
        kern, self.width, self.orig, self.new = dsp.sinc_resample_kernel(self.orig_freq, self.new_freq)
        self._kern_host = torch.from_numpy(np.ascontiguousarray(kern))
        self._kern = None
        self._init_mel(16000)
        self.noiser = noiser

    def _k(self, device):
        if self._kern is None or self._kern.device != device:
            self._kern = self._kern_host.to(device)
        return self._kern

    def _out_len(self, n):
        return int(math.ceil(self.new * n / self.orig))

    def apply(self, x, length, **kw):
        k = self._k(x.device)

        def adjoint(dy, full):
            return _fir_bwd(dy, k, None, length, full, self.orig, self.new, self.width)
        return _fir_fwd(x, length, k, self._out_len(length), self.orig, self.new, self.width), adjoint


class MusicDereverberationOperator(_MelOperator):         # operator.py:208-250
    """forward = conv1d with a random impulse response.  The reference draws a NEW response from the global RNG on
    every forward call (operator.py:244-246), so the measurement and every guidance step see different responses;
    that is the default here too.  `fixed_ir=True` (extension) draws once and keeps it; `ir=` pins one call."""

    def __init__(self, ir_length=800, decay_factor=0.85, noiser=None, fixed_ir=False):
        self.ir_length, self.decay_factor, self.fixed_ir = ir_length, decay_factor, fixed_ir
        self._init_mel(16000)
        self.noiser = noiser
        self._ir = None

    def generate_impulse_response(self, ir_length=800, decay_factor=0.85):       # operator.py:238-242 (host, global RNG)
        ir = torch.randn(ir_length)
        ir = torch.cumsum(ir, dim=0) * decay_factor
        ir /= ir.abs().max()
        return ir.unsqueeze(0)

    def _get_ir(self, device, ir=None):
        if ir is None:
            if self.fixed_ir and self._ir is not None:
                ir = self._ir
            else:
                ir = self.generate_impulse_response(self.ir_length, self.decay_factor)
                if self.fixed_ir:
                    self._ir = ir
        h = ir.reshape(1, -1).to(device=device, dtype=torch.float32).contiguous()
        return h, torch.flip(h, dims=[1]).contiguous()

    def apply(self, x, length, ir=None, **kw):
        """ir: the response of this call; None draws one (or takes the kept one of `fixed_ir`) before anything else happens."""
        h, h_rev = self._get_ir(x.device, ir)
        n = h.shape[1]

        def adjoint(dy, full):
            return _fir_bwd(dy, h, h_rev, length, full, 1, 1, n // 2)
        return _fir_fwd(x, length, h, length + 2 * (n // 2) - n + 1, 1, 1, n // 2), adjoint


class TimeFrequencyMaskOperator(_MelOperator):
    """Time-frequency masking (extension; every operator of the reference acts on the time axis): a real gain G[k, t] on the STFT of the
    clip, resynthesised to a waveform -- spectral holes, hum removal, a band-stop or low-pass at any cut-off, bleed confined to a band.

        A = (1 / c) P^T W F^-1 G F W P      n_fft 1024, hop 256, periodic Hann w, the clip ZERO outside [0, L), c = sum_j w[n + 256 j]^2 = 1.5

    Frame t = 0 .. T - 1, T = ceil(L / 256) + 3 = `dsp.tf_frames(L)`, covers the samples (t - 3) * 256 + n, n = 0 .. 1023, so every sample lies
    in exactly four frames; G = 1 gives A = I, and A is real and symmetric: `adjoint` is the same kernel (csrc/tf_gain.hip, DESIGN.md section
    8.7).  forward = noiser(A(x)), transform = clamp(wav2mel, -80, 80) like the IdentityOperator's.  A is materialised (`_on_load` is None):
    a guided step is the identity's plus two launches.

    gain: (513, T) -- one grid for every clip -- or (B, 513, T), fp32, finite, any sign, in the layout of `stft_mag` (bins, frames);
    `dsp.tf_gain_grid` builds one from boxes.  The grid belongs to ONE clip length: `apply`, `forward` and `guidance` raise a ValueError
    naming the expected shape for any other (inside a TrackOperator build it for the track's length).  With per-clip gains the batch must be
    B, and the pipelines refuse `lanes > 1` and `shard=True` (the gains are indexed by batch position); a shared grid has no such state.

    dead_span: a sample whose four covering frames have gain exactly zero in every bin, for every clip, does not reach y, and its gradient
    is exactly zero.  Frames t0 .. t1 all zero, t1 - t0 >= 3, give the samples [256 t0, 256 (t1 - 2)); the longest such run is found on the
    host once.  The front end and the device copy are made on first use, so the operator can be built without a GPU."""

    def __init__(self, sample_rate, gain, noiser=None):
        g = torch.as_tensor(gain).detach().to(device="cpu", dtype=torch.float32)
        if g.dim() not in (2, 3) or g.shape[-2] != dsp.TF_BINS or g.shape[-1] < 4 or g.shape[0] < 1:
            raise ValueError(f"gain has shape {tuple(g.shape)}: ({dsp.TF_BINS}, T) for every clip or (B, {dsp.TF_BINS}, T), T = ceil(L / 256) + 3")
        if not bool(torch.isfinite(g).all()):
            raise ValueError("gain: finite values (a real gain per bin and frame, of any sign)")
        self.sample_rate, self.noiser = sample_rate, noiser
        self.per_clip = g.dim() == 3
        self.gain = g.clone()                                 # host copy, public layout (bins, frames)
        self._gain_t = None                                   # device copy as the kernel reads it: (frames, bins) rows
        self._dead = self._find_dead(g)
        self._init_mel(sample_rate, lazy=True)

    @property
    def frames(self):
        return self.gain.shape[-1]

    @property
    def positional_state(self):                               # one shared grid has no per-position state
        return ("TimeFrequencyMaskOperator with per-clip gains", "gains") if self.per_clip else None

    @staticmethod
    def _find_dead(g):
        """Frames whose gain is zero in every bin of every clip -> the longest run t0 .. t1 with t1 - t0 >= 3 as samples, or None."""
        zero = (g == 0).reshape(-1, g.shape[-2], g.shape[-1]).all(dim=1).all(dim=0)
        run = longest_zero_run(torch.where(zero, 0.0, 1.0).numpy())
        if run is None or run[1] - run[0] < 4:
            return None
        return dsp.TF_HOP * run[0], dsp.TF_HOP * (run[1] - 3)  # t1 = run[1] - 1 inclusive: [256 t0, 256 (t1 - 2))

    def dead_span(self, length):
        if self._dead is None or dsp.tf_frames(length) != self.frames:
            return None
        s0, s1 = self._dead[0], min(self._dead[1], int(length))
        return (s0, s1) if s1 > s0 else None

    def _check(self, batch, length):
        T = dsp.tf_frames(length)
        if self.frames != T:
            raise ValueError(f"TimeFrequencyMaskOperator holds a gain of shape {tuple(self.gain.shape)}; a clip of {length} samples needs "
                             f"({dsp.TF_BINS}, {T}) = (513, ceil({length} / 256) + 3)")
        if self.per_clip and self.gain.shape[0] != batch:
            raise ValueError(f"TimeFrequencyMaskOperator holds {self.gain.shape[0]} per-clip gain(s) of shape ({dsp.TF_BINS}, {T}), the batch "
                             f"has {batch} clip(s): expected ({batch}, {dsp.TF_BINS}, {T})")

    def gain_on(self, device):
        """The gain on `device` as the kernel reads it, (T, 513) or (B, T, 513) contiguous (one tensor, kept)."""
        if self._gain_t is None or self._gain_t.device != device:
            self._gain_t = self.gain.transpose(-1, -2).contiguous().to(device)
        return self._gain_t

    def forward(self, data, **kwargs):
        self._check(data.shape[0], data.shape[-1])            # before the tensor has to be on the GPU
        return super().forward(data, **kwargs)

    def guidance(self, wav, length, measurement, supervised_space, **kw):
        self._check(wav.shape[0], length)
        return super().guidance(wav, length, measurement, supervised_space, **kw)

    def apply(self, x, length, **kw):
        self._check(x.shape[0], length)
        h, g = self.frontend._h.value, self.gain_on(x.device)

        def adjoint(dy, full):                                # A is symmetric: the transpose is A, zero-padded to `full`
            return ops.hip.tf_gain(h, dy.contiguous(), g, int(length), int(full))
        return ops.hip.tf_gain(h, x, g, int(length), int(length)), adjoint


class CodecOperator(_MelOperator):
    """Codec restoration (extension; the first nonlinearity in a TRANSFORM domain, with a gate on every coefficient): the measurement of a
    lossy codec -- MP3, AAC, Vorbis -- is an MDCT of the signal whose coefficients were quantised, one step per band and frame, everything
    above a cut-off thrown away.  Per clip, x zero outside [0, L) (csrc/mdct_quant.hip):

        A = Phi^T Q Phi      Phi: MDCT, N = 512 coefficients per frame, frame length 1024, hop 512, window sin(pi (n + 1/2) / 1024),
                             T = ceil(L / 512) + 1 = `dsp.mdct_frames(L)` frames, frame t at sample (t - 1) * 512; Phi^T Phi = I on the clip
        Q(C) = rint(C / D) D round-half-even; D = 0 is transparent, D = +inf discards the coefficient (the codec's low-pass)

    forward = noiser(A(x)), transform = clamp(wav2mel, -80, 80) like the IdentityOperator's.  A is materialised (`_on_load` is None): a guided
    step is the identity's plus one `mdct_quant` launch, and a second one where a step is infinite.

    STRAIGHT-THROUGH BACKWARD: Q is a staircase, its Jacobian is zero almost everywhere and useless for guidance.  `adjoint` replaces the
    staircase by its mean slope -- 1 on a kept coefficient, 0 on a discarded one: adjoint(dy) = Phi^T K Phi dy, K[k, t] = [D[k, t] < inf].
    It is symmetric, linear in dy and independent of x.  Where no step of the grid is infinite it is the identity on the clip: `adjoint` is
    then the zero-padded copy and launches no transform.  The gradient `guidance` returns is therefore NOT the derivative of its loss.

    step: (512, T) -- one grid for every clip -- or (B, 512, T), fp32, 0 <= D <= +inf, in the layout of the time-frequency gain (coefficients,
    frames); `dsp.codec_step_grid` and `dsp.codec_steps_for_nmr` build one.  A negative or NaN step is refused by name.  The grid belongs to
    ONE clip length: `apply`, `forward`, `guidance`, `encode` and `project` raise a ValueError naming the expected shape for any other (inside
    a TrackOperator build it for the track's length).  With per-clip grids the batch must be B, and the pipelines refuse `lanes > 1` and
    `shard=True` (the grids are indexed by batch position); a shared grid has no such state.

    dead_span: frames t0 .. t1 whose steps are +inf in every coefficient, for every clip, leave the samples [512 t0, 512 t1) -- those that
    only these frames cover -- exactly +0 in y and in the gradient; the longest such run is found on the host once.  `project` is the optional
    output stage.  The front end and the device copy are made on first use, so the operator can be built without a GPU."""

    def __init__(self, sample_rate=16000, step=None, noiser=None):
        if step is None:
            raise ValueError(f"step: a ({dsp.MDCT_N}, T) grid for every clip or (B, {dsp.MDCT_N}, T), T = ceil(L / 512) + 1 (dsp.codec_step_grid)")
        d = torch.as_tensor(step).detach().to(device="cpu", dtype=torch.float32)
        if d.dim() not in (2, 3) or d.shape[-2] != dsp.MDCT_N or d.shape[-1] < 2 or d.shape[0] < 1:
            raise ValueError(f"step has shape {tuple(d.shape)}: ({dsp.MDCT_N}, T) for every clip or (B, {dsp.MDCT_N}, T), T = ceil(L / 512) + 1")
        if bool(torch.isnan(d).any()) or bool((d < 0).any()):
            raise ValueError("step: values in [0, +inf] (0 = transparent, +inf = the coefficient is discarded); negative or NaN steps are refused")
        self.sample_rate, self.noiser = sample_rate, noiser
        self.per_clip = d.dim() == 3
        self.step = d.clone()                                 # host copy, public layout (coefficients, frames)
        self._step_t = None                                   # device copy as the kernel reads it: (frames, coefficients) rows
        self.lossless = not bool(torch.isinf(d).any())        # no coefficient is discarded: the straight-through transpose is the identity
        self._dead = self._find_dead(d)
        self._init_mel(sample_rate, lazy=True)

    @property
    def step_frames(self):
        return self.step.shape[-1]

    def frames(self, length):
        return dsp.mdct_frames(length)

    @property
    def positional_state(self):                               # one shared grid has no per-position state
        return ("CodecOperator with per-clip step grids", "step grids") if self.per_clip else None

    @staticmethod
    def _find_dead(d):
        """Frames whose step is +inf in every coefficient of every clip -> the longest run t0 .. t1, t1 > t0, as samples [512 t0, 512 t1)."""
        gone = torch.isinf(d).reshape(-1, d.shape[-2], d.shape[-1]).all(dim=1).all(dim=0)
        run = longest_zero_run(torch.where(gone, 0.0, 1.0).numpy())
        if run is None or run[1] - run[0] < 2:
            return None
        return dsp.MDCT_N * run[0], dsp.MDCT_N * (run[1] - 1)   # t1 = run[1] - 1 inclusive

    def dead_span(self, length):
        if self._dead is None or dsp.mdct_frames(length) != self.step_frames:
            return None
        s0, s1 = self._dead[0], min(self._dead[1], int(length))
        return (s0, s1) if s1 > s0 else None

    def _check(self, batch, length):
        T = dsp.mdct_frames(length)
        if self.step_frames != T:
            raise ValueError(f"CodecOperator holds a step grid of shape {tuple(self.step.shape)}; a clip of {length} samples needs "
                             f"({dsp.MDCT_N}, {T}) = (512, ceil({length} / 512) + 1)")
        if self.per_clip and self.step.shape[0] != batch:
            raise ValueError(f"CodecOperator holds {self.step.shape[0]} per-clip step grid(s) of shape ({dsp.MDCT_N}, {T}), the batch "
                             f"has {batch} clip(s): expected ({batch}, {dsp.MDCT_N}, {T})")

    def step_on(self, device):
        """The step grid on `device` as the kernel reads it, (T, 512) or (B, T, 512) contiguous (one tensor, kept)."""
        if self._step_t is None or self._step_t.device != device:
            self._step_t = self.step.transpose(-1, -2).contiguous().to(device)
        return self._step_t

    def forward(self, data, **kwargs):
        self._check(data.shape[0], data.shape[-1])            # before the tensor has to be on the GPU
        return super().forward(data, **kwargs)

    def guidance(self, wav, length, measurement, supervised_space, **kw):
        self._check(wav.shape[0], length)
        return super().guidance(wav, length, measurement, supervised_space, **kw)

    def apply(self, x, length, **kw):
        self._check(x.shape[0], length)
        h, d = self.frontend._h.value, self.step_on(x.device)

        def adjoint(dy, full):                                # straight-through: Phi^T K Phi, the zero-padded copy where K = 1 everywhere
            if self.lossless:
                return ops.hip.mask_mul(dy, None, int(length), int(full))
            return ops.hip.mdct_quant(h, dy.contiguous(), d, int(length), int(full), passthrough=True)[0]
        return ops.hip.mdct_quant(h, x, d, int(length), int(length))[0], adjoint

    def _rows(self, audio):
        """audio as (B, L) fp32 rows on the GPU, checked against the grid first"""
        a = torch.as_tensor(audio)
        a = a.reshape(a.shape[0], -1)
        self._check(a.shape[0], a.shape[1])                   # before the tensor has to be on the GPU
        a = _as_f32_cuda(a)
        return a if a.stride(1) == 1 else a.contiguous()

    def encode(self, audio):
        """audio (B, L) -> the codes rint(Phi audio / D) as (B, T, 512) int32; INT32_MIN marks a coefficient that is not coded (D = 0, or a
        quotient of 2^23 and more), a discarded one has code 0."""
        a = self._rows(audio)
        return ops.hip.mdct_quant(self.frontend._h.value, a, self.step_on(a.device), a.shape[1], a.shape[1], want_codes=True)[1]

    def project(self, wav, measurement):
        """The conventional output stage of codec restoration -> (B, L), L the measurement's length: the MDCT coefficients of the restored
        audio are clamped into the quantiser cells [(q - 1/2) D, (q + 1/2) D] of the measurement's codes q = rint(Phi y / D), and
        resynthesised.  Only on WHOLE frames (1 <= t <= L // 512 - 1: all 1024 samples inside the clip), where Phi Phi^T = I and the codes of
        the measurement are the codec's own; the two edge frames, transparent, discarded and uncoded coefficients are left as they are.
        Opt-in; refused with measurement noise, under which the codes of y are not the codec's."""
        if step_sigma(self.noiser) > 0:
            raise ValueError("project: the measurement carries additive noise (sigma > 0), so its codes are not the codec's")
        y = self._rows(measurement)
        wav = _as_f32_cuda(torch.as_tensor(wav).to(y.device))
        wav = wav.reshape(wav.shape[0], -1)
        if wav.shape[0] != y.shape[0] or wav.shape[1] < y.shape[1]:
            raise ValueError(f"project: restored audio {tuple(wav.shape)} does not cover the measurement {tuple(y.shape)}")
        if wav.stride(1) != 1:
            wav = wav.contiguous()
        h, d, L_ = self.frontend._h.value, self.step_on(y.device), y.shape[1]
        codes = ops.hip.mdct_quant(h, y, d, L_, L_, want_codes=True)[1]
        return ops.hip.mdct_project(h, wav, d, codes, L_, L_)


class DynamicRangeOperator(_MelOperator):
    """De-compression (extension; the first operator that is nonlinear WITH MEMORY): a feed-forward, mono dynamic-range compressor or
    limiter -- over-mastered releases, broadcast AGC, bus compressors -- whose sidechain runs on blocks of 64 samples (4 ms at 16 kHz).
    Per clip, x zero outside [0, L) (csrc/drc.hip):

        p[j] = mean of x^2 over block j     d = 10 log10(p + 1e-10) - threshold_db     k = 1 - 1 / ratio, W = knee_db
        c[j] = 0 (2 d < -W) | k (d + W/2)^2 / (2 W) (2 d <= W) | k d                   the static curve: gain reduction in dB
        s[j] = s[j-1] + (c[j] > s[j-1] ? aA : aR) (c[j] - s[j-1]), s[-1] = 0           aA, aR = dsp.drc_coeffs(sample_rate, attack_ms, release_ms)
        G[j] = 10^((makeup_db - s[j]) / 20)                                            y = g x, g linear from G[j-1] to G[j] over block j

    forward = noiser(A(x)), transform = clamp(wav2mel, -80, 80) like the IdentityOperator's.  A is materialised (`_on_load` is None): a
    guided step is the identity's plus `drc_fwd` and `drc_bwd`, three launches each.  The Jacobian is not diagonal: `adjoint` runs the
    follower's recurrence backwards in time, at the x `apply` was given, with the gates `apply` decided (one tape byte per block).

    The parameters are GIVEN, shared by all clips and rounded to fp32 once here; nothing is fitted and nothing is kept per clip, so clip lanes
    and sharding work.  ratio = inf is a limiter.  Bad parameters are refused by name at construction; the front end is made on first use, so
    the operator can be built without a GPU.  `dead_span` is None: every sample reaches y."""

    def __init__(self, sample_rate=16000, threshold_db=-24.0, ratio=4.0, knee_db=6.0, attack_ms=5.0, release_ms=100.0, makeup_db=0.0, noiser=None):
        def finite(name, v, lo=None, hi=200.0):
            v = float(v)
            if not math.isfinite(v) or abs(v) > hi or (lo is not None and v < lo):
                raise ValueError(f"{name} = {v!r}: a finite number" + (f" >= {lo}" if lo is not None else "") + f", at most {hi} in magnitude")
            return float(np.float32(v))
        if not (math.isfinite(float(sample_rate)) and float(sample_rate) > 0):
            raise ValueError(f"sample_rate = {sample_rate!r}: a positive finite rate")
        ratio = float(ratio)
        if math.isnan(ratio) or ratio < 1:
            raise ValueError(f"ratio = {ratio!r}: at least 1 (inf = a limiter)")
        self.sample_rate, self.noiser = sample_rate, noiser
        self.threshold_db, self.makeup_db = finite("threshold_db", threshold_db), finite("makeup_db", makeup_db)
        self.knee_db = finite("knee_db", knee_db, lo=0.0)
        self.ratio, self.attack_ms, self.release_ms = ratio, float(attack_ms), float(release_ms)
        self.slope = float(np.float32(1.0 - 1.0 / ratio))         # k
        a_att, a_rel = dsp.drc_coeffs(sample_rate, attack_ms, release_ms)      # refuses bad times by name
        self.a_att, self.a_rel = float(a_att), float(a_rel)
        self._init_mel(sample_rate, lazy=True)

    @property
    def params(self):
        """The six fp32 parameters in the order `drc_fwd` / `drc_bwd` take them."""
        return self.threshold_db, self.slope, self.knee_db, self.a_att, self.a_rel, self.makeup_db

    def apply(self, x, length, **kw):
        params = self.params
        y, state, tape = ops.hip.drc_fwd(x, int(length), *params)

        def adjoint(dy, full):                                # the Jacobian of a nonlinear A is taken at x, with the gates of this apply
            return ops.hip.drc_bwd(dy, x, state, tape, int(full), *params)
        return y, adjoint


class TimeWarpOperator(_MelOperator):
    """Wow and flutter (extension; the first operator that MOVES samples in time): the playback speed was not the recording speed, and it
    varied -- tape, cassette, vinyl and film transfers.  Per clip, x zero outside [0, L) (csrc/warp.hip):

        delta(64 j + r) = d[j] + (r / 64) (d[j+1] - d[j])      the delay curve: H + 1 = dsp.warp_knots(L) knots in samples, one per 64 samples
        y[n] = x(n + delta(n))                                 four-point Catmull-Rom on the taps i - 1 .. i + 2, i = n + floor(delta)

    Positive delta reads ahead: the medium ran fast.  forward = noiser(A(x)), transform = clamp(wav2mel, -80, 80) like the
    IdentityOperator's.  A is linear and materialised (`_on_load` is None): a guided step is the identity's plus `warp_fwd` and `warp_bwd`,
    one launch each; `adjoint` is the transpose as a gather, without atomics.

    delay: (H + 1,) -- one curve for every clip -- or (B, H + 1), fp32 knots; `dsp.wow_curve` builds one from speed components.  It is GIVEN,
    not fitted, and checked here, by name, on the host copy: finite, |d[j]| <= 4096, |d[j+1] - d[j]| <= 16.  The curve belongs to ONE clip
    length: `apply`, `forward` and `guidance` raise a ValueError naming `warp_knots(length)` for any other (inside a TrackOperator build it
    for the track's length).  With per-clip curves the batch must be B, and the pipelines refuse `lanes > 1` and `shard=True` (the curves
    are indexed by batch position); a shared curve has no such state.  The front end and the device copy are made on first use, so the
    operator can be built without a GPU.  `dead_span` is None: the curve moves every sample."""

    def __init__(self, sample_rate=16000, delay=None, noiser=None):
        if not (math.isfinite(float(sample_rate)) and float(sample_rate) > 0):
            raise ValueError(f"sample_rate = {sample_rate!r}: a positive finite rate")
        if delay is None:
            raise ValueError("delay: the knots of the delay curve, (warp_knots(length),) or (B, warp_knots(length)) (dsp.wow_curve builds one)")
        d = torch.as_tensor(delay).detach().to(device="cpu", dtype=torch.float32).contiguous()
        dsp.check_warp_curve(d.numpy(), "delay")
        self.sample_rate, self.noiser = sample_rate, noiser
        self.per_clip = d.dim() == 2
        self.delay = d.clone()                                # host copy
        self._delay_dev = None
        self._init_mel(sample_rate, lazy=True)

    @property
    def knots(self):
        return self.delay.shape[-1]

    @property
    def positional_state(self):                               # one shared curve has no per-position state
        return ("TimeWarpOperator with per-clip delay curves", "curves") if self.per_clip else None

    def _check(self, batch, length):
        K = dsp.warp_knots(length)
        if self.knots != K:
            raise ValueError(f"TimeWarpOperator holds a delay curve of shape {tuple(self.delay.shape)}; a clip of {length} samples needs "
                             f"warp_knots({length}) = {K} knots")
        if self.per_clip and self.delay.shape[0] != batch:
            raise ValueError(f"TimeWarpOperator holds {self.delay.shape[0]} per-clip delay curve(s), the batch has {batch} clip(s): expected "
                             f"({batch}, {K})")

    def delay_on(self, device):
        """The knots on `device` (one tensor, kept)."""
        if self._delay_dev is None or self._delay_dev.device != device:
            self._delay_dev = self.delay.to(device)
        return self._delay_dev

    def forward(self, data, **kwargs):
        self._check(data.shape[0], data.shape[-1])            # before the tensor has to be on the GPU
        return super().forward(data, **kwargs)

    def guidance(self, wav, length, measurement, supervised_space, **kw):
        self._check(wav.shape[0], length)
        return super().guidance(wav, length, measurement, supervised_space, **kw)

    def apply(self, x, length, **kw):
        self._check(x.shape[0], length)
        d = self.delay_on(x.device)

        def adjoint(dy, full):                                # A is linear: the transpose needs neither x nor a tape
            return ops.hip.warp_bwd(dy.contiguous(), d, int(length), int(full))
        return ops.hip.warp_fwd(x, d, int(length)), adjoint


class DeclickOperator(_MelOperator):
    """Declicking (extension): impulsive noise -- clicks, crackle, ticks, digital dropouts -- of a vinyl, tape or cassette transfer.  The
    model is y = x + sigma z + clicks with clicks nobody knows: the damaged samples are FOUND, by the autoregressive detector of
    csrc/declick.hip (a click is a sample the recent past cannot predict), and hidden from the loss by a 0/1 mask m
    with one row per clip.  The mask is a weight of the loss, not part of the degradation, so both sides carry it:

        wav_form          || m (x^ + sigma z - y) ||
        mel_spectrogram   || T(m y) - T(m (x^ + sigma z)) ||      T = clamp(wav2mel, -80, 80) like the IdentityOperator's

    The step's noise is added BEFORE the mask.  A is materialised (`_on_load` is None): a guided step is the identity's plus two `mask_rows`
    launches.  `forward(data, clicks=None)` = noiser(data + clicks) makes a synthetic measurement (`dsp.click_train` draws the clicks).

    The mask: with mask=None it is detected from the measurement on its first use and kept WITH the reference transform -- one entry of
    `BaseOperator._ref`'s cache holds both, so the rule is the same (keyed by the measurement tensor and its version, four entries,
    `cache_reference=False` re-detects every step).  It is a function of the measurement's rows alone: no positional state, so clip lanes
    and sharding work, and inside a TrackOperator detection runs on the (1, T) track.  `mask=` pins one instead: (L,) for every clip or
    (B, L), values 0 / 1, checked here by name; a (B, L) one is indexed by batch position (`positional_state`).  `last_masked_fraction` is
    the share of zeros of the last detection: one host read per detection, never per step.

    Limits: percussive onsets can be flagged (`threshold` is the knob); detection happens once, from y alone; bursts much longer than the
    model order (16 samples) are a job for the inpainting or time-frequency-mask operators.  `dead_span` is None."""

    def __init__(self, sample_rate=16000, threshold=5.0, sigma_floor=1e-5, guard=3, mask=None, noiser=None):
        if not (math.isfinite(float(sample_rate)) and float(sample_rate) > 0):
            raise ValueError(f"sample_rate = {sample_rate!r}: a positive finite rate")
        self.threshold, self.sigma_floor, self.guard = dsp.check_declick(threshold, sigma_floor, guard)
        self.sample_rate, self.noiser = sample_rate, noiser
        self.mask = None
        if mask is not None:
            m = torch.as_tensor(mask).detach().to(device="cpu")
            if m.dim() not in (1, 2) or m.numel() < 1:
                raise ValueError(f"mask has shape {tuple(m.shape)}: (L,) for every clip or (B, L)")
            if not bool(((m == 0) | (m == 1)).all()):
                raise ValueError("mask: values 0 (hidden from the loss) or 1 (kept)")
            self.mask = m.to(torch.float32).contiguous().clone()      # host copy
        self._mask_dev = None
        self.last_masked_fraction = None
        self._init_mel(sample_rate, lazy=True)

    @property
    def positional_state(self):                               # a detected or shared mask has no per-position state
        return ("DeclickOperator with a per-clip mask", "mask rows") if self.mask is not None and self.mask.dim() == 2 else None

    def forward(self, data, clicks=None, **kwargs):
        data = _as_f32_cuda(data)
        if clicks is not None:
            data = data + torch.as_tensor(clicks).to(device=data.device, dtype=torch.float32)
        return self._measure(data)

    def detect(self, measurement):
        """measurement (B, L) (or (B, 1, L)) on the GPU -> the (B, L) fp32 mask, 0 within `guard` samples of a detected click; sets
        `last_masked_fraction` (one host read)."""
        y = _as_f32_cuda(measurement)
        y = y.reshape(y.shape[0], -1)
        flags = ops.hip.click_detect(y, y.shape[1], self.threshold, self.sigma_floor)[3]
        mask, masked = ops.hip.click_mask(flags, self.guard)
        self.last_masked_fraction = float(masked.sum().item()) / float(mask.numel())
        return mask

    def _pinned(self, batch, length, device):
        m = self.mask
        if m.shape[-1] != length or (m.dim() == 2 and m.shape[0] != batch):
            raise ValueError(f"DeclickOperator holds a mask of shape {tuple(m.shape)}; {batch} clip(s) of {length} samples need ({length},) "
                             f"or ({batch}, {length})")
        if self._mask_dev is None or self._mask_dev.device != device:
            self._mask_dev = m.to(device)
        return self._mask_dev

    def mask_of(self, measurement):
        """The pinned mask on the measurement's device, or a fresh detection (no cache)."""
        y = measurement.reshape(measurement.shape[0], -1)
        return self._pinned(y.shape[0], y.shape[1], y.device) if self.mask is not None else self.detect(y)

    def _entry(self, measurement, space, fn):
        """One cache entry per measurement and space: (mask, fn(mask * measurement))."""
        def make(y):
            y = y.reshape(y.shape[0], -1)
            m = self.mask_of(y)
            return m, fn(ops.hip.mask_rows(y, m, y.shape[1], y.shape[1]))
        return BaseOperator._ref(self, measurement, space, make)

    _step_entry = None                                       # (measurement, space, entry) while `guidance` runs: one detection per step

    def _ref(self, measurement, space, fn):
        held = self._step_entry
        if held is not None and held[0] is measurement and held[1] == space:
            return held[2][1]
        return self._entry(measurement, space, fn)[1]

    def guidance(self, wav, length, measurement, supervised_space, **kw):
        if supervised_space not in ("wav_form", "mel_spectrogram"):
            raise ValueError("supervised_space should be either 'wav_form' or 'mel_spectrogram")
        fn = _flat_rows if supervised_space == "wav_form" else (lambda m: self._mel(m).clone())
        entry = self._entry(measurement, supervised_space, fn)
        m = entry[0]
        if m.shape[-1] != length or (m.dim() == 2 and m.shape[0] != wav.shape[0]):
            raise ValueError(f"the click mask has shape {tuple(m.shape)}, the batch {wav.shape[0]} clip(s) of {length} samples")
        self._step_entry = (measurement, supervised_space, entry)      # with cache_reference=False too, the step detects once
        try:
            return super().guidance(wav, length, measurement, supervised_space, mask=m, **kw)
        finally:
            self._step_entry = None

    def apply(self, x, length, mask=None, **kw):
        """y = mask * x[:, :length]; `mask` (L,) or (B, L) on x's device -- `guidance` hands over the measurement's."""
        if mask is None:
            if self.mask is None:
                raise ValueError("DeclickOperator.apply: mask= is needed (the detected mask belongs to a measurement; `guidance` passes it)")
            mask = self._pinned(x.shape[0], int(length), x.device)

        def adjoint(dy, full):                                # a per-sample mask is its own transpose
            return ops.hip.mask_rows(dy, mask, int(length), int(full))
        return ops.hip.mask_rows(x, mask, int(length), int(length)), adjoint

    def _noisy_apply(self, wav, length, noise, step, generator, **apply_kw):
        """The step's noise enters BEFORE the mask: y = mask * (wav[:, :length] + sigma z); the transpose is unchanged."""
        z, sigma = self._step_noise((wav.shape[0], int(length)), wav.device, noise, step, generator)
        if z is not None:
            wav = ops.hip.noise_add(ops.hip.mask_mul(wav, None, int(length), int(length)), z, sigma)
        return self.apply(wav, length, **apply_kw)

    def project(self, audio, measurement, fade=16):
        """The optional output stage -> (B, L), L the measurement's length: the measurement's own samples, bit for bit, away from the
        mask's zeros; the restored `audio` on them; a linear cross-fade over `fade` samples (0 .. 64) on each side.  Meaningful after
        `wav_form` guidance only: mel guidance does not fix the phase, so a restored stretch need not line up with its surroundings."""
        fade = dsp.check_declick_fade(fade)
        y = _as_f32_cuda(measurement)
        y = y.reshape(y.shape[0], -1)
        x = _as_f32_cuda(torch.as_tensor(audio).to(y.device))
        x = x.reshape(x.shape[0], -1)
        if x.shape[0] != y.shape[0] or x.shape[1] < y.shape[1]:
            raise ValueError(f"project: restored audio {tuple(x.shape)} does not cover the measurement {tuple(y.shape)}")
        if x.stride(1) != 1:
            x = x.contiguous()
        m = None
        if self.mask is None and self.cache_reference:        # the mask this trajectory used, when it is still cached
            for c in self._ref_cache or []:
                if c[0] is measurement and c[1] == measurement._version:
                    m = c[3][0]
                    break
        if m is None:
            m = self.mask_of(y)
        return ops.hip.declick_blend(x, y, m, y.shape[1], fade)


class StyleGuidanceOperator(BaseOperator):               # operator.py:253-271 (unrunnable in the reference: run.py:213-214)
    """Style guidance with BUILD-DEFINED semantics (the reference's `clap_model.get_gram_matrix`
    does not exist anywhere): `forward(x) = noiser(x)` (identity, operator.py:270-271) and

        transform(audio) = Gram(F) = F F^T / T,   F = CLAP (HTS-AT) audio-encoder token features (B, C, T) of the waveform

    computed as: 16 kHz -> 48 kHz sinc-hann polyphase resampling (HIP `dmx_fir_fwd`), CLAP's log-mel front end (48 kHz,
    n_fft 1024, hop 480, 64 slaney mel bins 0-14 kHz, power dB; HIP `dmx_audio_transform_fwd`), then the HTS-AT tower
    (`transformers.ClapAudioModel` weights) on the hand-written executor `HtsatEngine` (csrc/htsat.hip: forward with tape and
    input-gradient backward on the library's GEMM / LayerNorm / window-attention kernels), the Gram matrix and its gradient
    (`dmx_gram_fwd` / `dmx_gram_bwd`) and the per-clip L2 loss: the whole guidance pair is HIP.  `tower="torch"` runs the wrapped
    torch module through autograd instead (the round-4 path, kept for A/B measurements only).
    Loss = ||G(y) - G(x_hat)||_2 per clip."""

    def __init__(self, sample_rate=16000, clap_model=None, noiser=None, device="cuda", seed=0, tower="hip"):
        if tower not in ("hip", "torch"):
            raise ValueError("tower: 'hip' (HtsatEngine) or 'torch' (wrapped module, autograd)")
        self.sample_rate, self.noiser, self.tower = sample_rate, noiser, tower
        self.clap_sr, self.max_samples = 48000, 480000
        kern, self.width, self.orig, self.new = dsp.sinc_resample_kernel(sample_rate, self.clap_sr)
        self._kern_host, self._kern = torch.from_numpy(np.ascontiguousarray(kern)), None
        from transformers.audio_utils import mel_filter_bank
        fb = mel_filter_bank(num_frequency_bins=513, num_mel_filters=64, min_frequency=0.0, max_frequency=14000.0, sampling_rate=48000,
                             norm="slaney", mel_scale="slaney")                    # ClapFeatureExtractor.mel_filters_slaney
        self.frontend = SpectralFrontend(self.clap_sr, 1024, 480, 64, "hann", fb=fb)
        if clap_model is None:                                                     # no checkpoint offline: seeded random HTS-AT
            from transformers import ClapAudioConfig, ClapAudioModel
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(seed)
                clap_model = ClapAudioModel(ClapAudioConfig())
        self.clap = getattr(clap_model, "audio_model", clap_model).to(device).float().eval()
        for p in self.clap.parameters():
            p.requires_grad_(False)
        self.engine = None
        if tower == "hip":
            from ..engine import HtsatEngine
            self.engine = HtsatEngine(self.clap.config, device=device).load_state_dict(self.clap.state_dict(), strict=True)

    def _k(self, device):
        if self._kern is None or self._kern.device != device:
            self._kern = self._kern_host.to(device)
        return self._kern

    def apply(self, x, length, **kw):
        return _masked(x, length, None)

    def _features(self, wav, length):
        """(B, >= length) fp32 cuda -> CLAP input features (B, 1, frames, 64) (HIP) and the 48 kHz length."""
        n48 = int(math.ceil(self.new * length / self.orig))
        x48 = _fir_fwd(wav, length, self._k(wav.device), n48, self.orig, self.new, self.width)
        mel = self.frontend.transform_fwd(x48, n48, True, True)                    # (B, frames, 64) log-mel dB
        return mel[:, None], n48

    def _gram(self, feats):
        if self.engine is not None:
            from ..engine import gram
            return gram(self.engine.forward(feats[:, 0].contiguous(), keep_state=False))
        f = self.clap(input_features=feats, is_longer=None, return_dict=True).last_hidden_state.flatten(2)   # (B, C, T)
        return torch.bmm(f, f.transpose(1, 2)) / f.shape[2]

    def _tower_guidance(self, feats, ref):
        """loss[b] = ||ref[b] - Gram(tower(feats[b]))||_2 and d loss / d feats, all HIP: tower forward (tape), Gram, L2 loss + its gradient,
        Gram transpose, per-clip rescale of the cotangent to the 16-bit range of the tower's backward sweep (undone on its output)."""
        from ..engine import gram, gram_backward
        f = self.engine.forward(feats[:, 0].contiguous(), keep_state=True)           # (B, 64, 768) fp32
        g = gram(f)
        B = g.shape[0]
        loss, dg = l2_loss(ref.reshape(ref.shape[0], -1), g.reshape(B, -1))
        df = gram_backward(f, dg.reshape(g.shape))
        inv_scale = ops.hip.grad_normalize_(df.reshape(B, -1), 64.0)          # in place on df
        return loss, self.engine.backward(df, scale=inv_scale)[:, None]

    @torch.no_grad()
    def transform(self, audio):
        audio = _as_f32_cuda(audio)
        feats, _ = self._features(audio.contiguous(), audio.shape[-1])
        return self._gram(feats)

    def _mel_guidance(self, wav, length, measurement, noise, step, generator, **apply_kw):
        y = wav                                                    # the resampler reads wav[:, :length] in place: only the noise needs the crop
        z, sigma = self._step_noise((wav.shape[0], length), wav.device, noise, step, generator)
        if z is not None:
            y = ops.hip.noise_add(self.apply(wav, length)[0], z, sigma)
        ref = self._ref(measurement, "mel_spectrogram", lambda m: self.transform(m.reshape(m.shape[0], -1)))
        feats, n48 = self._features(y, length)
        if self.engine is not None:
            loss, dfeat = self._tower_guidance(feats, ref)
        else:
            with torch.enable_grad():
                fg = feats.detach().requires_grad_(True)
                diff = (ref - self._gram(fg)).flatten(1)
                loss = torch.linalg.vector_norm(diff, dim=1)                        # per-clip Frobenius norm
                (dfeat,) = torch.autograd.grad(loss.sum(), fg)
        dx48 = self.frontend.transform_bwd(dfeat[:, 0].contiguous())              # (B, n48)
        dwav = _fir_bwd(dx48, self._k(wav.device), None, length, wav.shape[1], self.orig, self.new, self.width)
        return loss.detach(), dwav
