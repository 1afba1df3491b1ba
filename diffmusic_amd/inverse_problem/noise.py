"""Measurement noise (reference: diffmusic/inverse_problem/noise.py).

A noiser is called by `operator.forward` when the user builds the measurement, and -- when it has an additive Gaussian part
(`additive_sigma > 0`) -- by every guided step, where the reference's schedulers call `operator.forward` on the predicted audio
(scheduling_dps.py:200 and siblings).  The per-step draw is made on the device by the in-tree Philox kernel (csrc/rng.hip), never by
`torch.randn` on the GPU."""
import torch

_MASK64 = 0xFFFFFFFFFFFFFFFF
MEASUREMENT_KEY_XOR = 0x6D6561735F6E6F69       # ASCII "meas_noi": separates the measurement-noise keys from the sampler's (csrc/rng.hip)
STREAMS = ("global", "clip")


def _signed64(v):
    """A 64-bit key as the signed value the op schema's int / int[] can carry (both bindings read it modulo 2^64)."""
    v &= _MASK64
    return v - (1 << 64) if v >= (1 << 63) else v


def clip_noise_key(seed, step):
    """(key, offset) of `randn_philox` for the measurement noise of a clip whose generator has initial seed `seed` at step index `step`
    (the position of the timestep in the scheduler's list, 0 = first step of the trajectory): element i of the draw is normal i & 3 of
    Philox block (step << 32) + i // 4 under key seed ^ MEASUREMENT_KEY_XOR."""
    return _signed64(int(seed) ^ MEASUREMENT_KEY_XOR), int(step) << 32


class BaseNoise:
    additive_sigma = 0.0      # > 0: the guided step adds additive_sigma * N(0, 1) to A(x); only noisers that say so take part in the step

    def __call__(self, data):
        return self.forward(data)

    def forward(self, data):
        raise NotImplementedError

    def reset(self):
        """A new trajectory starts (scheduler.set_timesteps)."""


class GaussianNoise(BaseNoise):               # noise.py:13-18
    """data + sigma * N(0, 1).  `forward` (building the measurement) draws from torch's global RNG like the reference.  Inside a guided
    step the draw comes from `draw`, on one of two streams:

    stream="global" (default; the reference's semantics: one process-wide stream consumed in call order): one Philox key is taken
        from torch's global CPU generator at the first noisy step of a trajectory, so `torch.manual_seed` reproduces a run; every
        call draws the whole (B, ...) tensor as one sequence and advances the offset.  The values depend on the batch a step holds,
        so the pipelines refuse this stream under clip lanes and clip sharding.
    stream="clip": clip k's noise at step i is a pure function of (initial seed of clip k's generator, i, element index) --
        `clip_noise_key` -- whatever the batch, lane or rank the clip runs in.  It needs the generator(s) given to the pipeline /
        `scheduler.step`; one shared generator keys clip k of the batch by initial_seed + k.  A NaN-retry restart of the pipeline
        replays the same measurement noise (the key holds the step index, not a call counter), while the latents are redrawn.

    sigma == 0 draws nothing, launches nothing and leaves the global RNG untouched."""

    def __init__(self, sigma, stream="global"):
        if stream not in STREAMS:
            raise ValueError(f"Unknown noise stream: {stream} (one of {STREAMS})")
        self.sigma = sigma
        self.stream = stream
        self._key = None
        self._offset = 0

    @property
    def additive_sigma(self):
        return float(self.sigma)

    def forward(self, data):
        if self.sigma == 0:
            return data
        return data + torch.randn_like(data) * self.sigma

    def reset(self):
        self._key = None
        self._offset = 0

    def draw(self, shape, device, step=None, generator=None):
        """Standard-normal (B, ...) fp32 tensor on `device` for one guided step (to be used as sigma * draw)."""
        from ..torch_utils import randn_philox
        B = int(shape[0])
        n = 1
        for d in shape[1:]:
            n *= int(d)
        if self.stream == "global":
            if self._key is None:
                self._key = _signed64(int(torch.randint(0, 2 ** 63 - 1, (1,)).item()) ^ MEASUREMENT_KEY_XOR)
            out = randn_philox((1, B * n), [self._key], self._offset, device).reshape(tuple(shape))
            self._offset += (B * n + 3) // 4
            return out
        if step is None or generator is None:
            raise ValueError("GaussianNoise(stream='clip') needs the step index and the clip generator(s): pass `generator=` to the "
                             "pipeline / scheduler.step (their initial seeds key the per-clip measurement noise)")
        shared = not isinstance(generator, (list, tuple))
        gens = [generator] * B if shared else list(generator)
        if len(gens) != B or any(g is None for g in gens):
            raise ValueError(f"GaussianNoise(stream='clip') needs one generator per clip: got {len(gens)} for batch {B}")
        keys = [clip_noise_key(int(g.initial_seed()) + (k if shared else 0), step) for k, g in enumerate(gens)]
        offset = keys[0][1]
        parts = [randn_philox((len(keys[lo:lo + 64]),) + tuple(shape[1:]), [k for k, _ in keys[lo:lo + 64]], offset, device)
                 for lo in range(0, B, 64)]             # one launch per 64 clips (the kernel's seed table); the seeds travel as kernel arguments
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)


class PoissonNoise(BaseNoise):                # noise.py:21-39 (not selected by any config; no additive part: stays out of the guided step)
    def __init__(self, rate):
        self.rate = rate

    def forward(self, data):
        d = ((data + 1.0) / 2.0).clamp(0, 1)
        d = torch.poisson(d * 255.0 * self.rate) / 255.0 / self.rate
        return (d * 2.0 - 1.0).clamp(-1, 1)


def step_sigma(noiser):
    """sigma of the additive Gaussian noise a guided step applies for this noiser (0.0: none -- no noiser, sigma 0, Poisson)."""
    return float(getattr(noiser, "additive_sigma", 0.0) or 0.0)
