"""CPU: the host side of the VAE encoder and of warm-started sampling (init audio / init mel + strength): exported and bound symbols
with the ABI version unchanged, the "rebuild" error for a version-4 library from before the encoder entry points, the strength rule of
the scheduler, the checkpoint reader's encoder keys, and the pipeline's argument rules and loop control on CPU stand-ins (the pattern
of tests/test_pipeline_host.py)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.stubs import SCHED, CpuPipeline, CpuScheduler, StubUNet, StubVae, StubVocoder

NEW_SYMBOLS = ("dmx_vae_encoder_create", "dmx_vae_encoder_workspace_bytes", "dmx_vae_encode_fwd", "dmx_latent_init")
N, B, SECONDS = 12, 3, 0.64            # 0.64 s -> mel height 64 -> latent (B, 8, 16, 4)


# ---- ABI --------------------------------------------------------------------------------------------------------------------------
def test_encoder_symbols_are_exported_and_bound_without_a_version_bump():
    from diffmusic_amd import _lib, ops
    from diffmusic_amd.build import build_library
    h = ctypes.CDLL(build_library())
    for name in NEW_SYMBOLS:
        assert hasattr(h, name), name
        assert name in _lib._SIGS, name
        assert name in _lib.ADDED_IN_V4, name
    h.dmx_abi_version.restype = ctypes.c_int
    assert h.dmx_abi_version() == 4 == _lib.ABI_VERSION
    assert "vae_enc_fwd" in ops.OP_NAMES and "latent_init" in ops.OP_NAMES


@pytest.mark.parametrize("missing", NEW_SYMBOLS)
def test_a_version_4_library_without_the_encoder_asks_for_a_rebuild(missing):
    """The additions did not move the ABI version, so an older build of the same version loads: the binding names what it lacks."""
    from diffmusic_amd import _lib
    old = SimpleNamespace(**{n: object() for n in _lib._SIGS if n != missing})
    with pytest.raises(RuntimeError, match=missing) as e:
        _lib.check_symbols(old, "libdiffmusic_hip.so")
    assert "rebuild" in str(e.value)
    _lib.check_symbols(SimpleNamespace(**{n: object() for n in _lib._SIGS}))          # a complete library passes


# ---- scheduler --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spacing", ["leading", "trailing", "linspace"])
def test_timesteps_for_strength_keeps_the_tail_of_the_full_list(spacing):
    from diffmusic_amd.schedulers.scheduling_guided import GuidedDDIMScheduler
    s = GuidedDDIMScheduler(**dict(SCHED, timestep_spacing=spacing, steps_offset=1 if spacing == "leading" else 0))
    s.set_timesteps(20)
    full = list(s._timesteps_host)
    for strength, keep in ((1.0, 20), (0.5, 10), (0.26, 5)):
        ts = s.timesteps_for_strength(strength)
        assert len(ts) == keep and ts == full[20 - keep:]
    assert s.num_inference_steps == 20 and list(s._timesteps_host) == full           # the list and the step width are untouched
    with pytest.raises(ValueError, match="strength"):
        s.timesteps_for_strength(0.04)
    with pytest.raises(ValueError, match="strength"):
        s.timesteps_for_strength(1.5)


# ---- checkpoint reader ------------------------------------------------------------------------------------------------------------
VAE = dict(_class_name="AutoencoderKL", act_fn="silu", block_out_channels=[64, 128, 256], down_block_types=["DownEncoderBlock2D"] * 3,
           in_channels=1, latent_channels=8, layers_per_block=2, norm_num_groups=32, out_channels=1, sample_size=512,
           scaling_factor=0.9, up_block_types=["UpDecoderBlock2D"] * 3)


def test_vae_config_reads_the_encoder_keys():
    from diffmusic_amd import checkpoint as ck
    v = ck.vae_config(VAE)
    assert v["block_out_channels"] == [64, 128, 256] and v["out_channels"] == 1 and v["latent_channels"] == 8
    with pytest.raises(ck.ConfigError, match="down_block_types"):
        ck.vae_config(dict(VAE, down_block_types=["DownEncoderBlock2D", "AttnDownEncoderBlock2D", "DownEncoderBlock2D"]))
    with pytest.raises(ck.ConfigError, match="down_block_types"):
        ck.vae_config(dict(VAE, down_block_types=["DownEncoderBlock2D"] * 2))
    with pytest.raises(ck.ConfigError, match="in_channels"):
        ck.vae_config(dict(VAE, in_channels=2))


# ---- pipeline (CPU stand-ins) -------------------------------------------------------------------------------------------------------
class StubDist:
    def __init__(self, mel):
        B = mel.shape[0]
        m = mel.reshape(B, 1, 16, 4, 4, 4).mean(dim=(3, 5))                        # (B, 1, 16, 4): the latent grid of a 64 x 16 mel
        self.mean = m.repeat(1, 8, 1, 1) * torch.arange(1, 9).reshape(1, 8, 1, 1) * 0.1
        self.logvar = torch.full_like(self.mean, -2.0)

    def mode(self, scale=1.0):
        return self.mean * scale

    def sample(self, generator=None, scale=1.0):
        from diffmusic_amd.torch_utils import randn_tensor
        return (self.mean + torch.exp(0.5 * self.logvar) * randn_tensor(self.mean.shape, generator=generator, dtype=torch.float32)) * scale


class StubEncoder:
    def __init__(self):
        self.calls, self.seen = 0, []

    def encode(self, mel, log_floor=0.0):
        self.calls += 1
        self.seen.append(mel.clone())
        return SimpleNamespace(latent_dist=StubDist(mel))


class WarmScheduler(CpuScheduler):
    def add_noise(self, original_samples, noise, timestep):                       # the product's formula without the HIP launch
        sa, s1 = self.add_noise_scalars(timestep)
        self.noised_at = getattr(self, "noised_at", []) + [int(timestep)]
        return sa * original_samples + s1 * noise


def make_pipeline(encoder=True, **sched_kw):
    pipe = CpuPipeline(StubVae(), StubUNet(), StubVocoder(), WarmScheduler(operator=None, **SCHED, **sched_kw),
                       vae_encoder=StubEncoder() if encoder else None).to("cpu")
    pipe.assume_uncond_equals_cond = True
    return pipe


def _args(**kw):
    g = torch.Generator().manual_seed(99)
    args = dict(prompt_embeds=torch.randn(B, 512, generator=g), audio_length_in_s=SECONDS, num_inference_steps=N, show_progress=False,
                generator=[torch.Generator().manual_seed(s) for s in range(B)], eta=0.0)
    args.update(kw)
    return args


def _mel(seed=3):
    return torch.randn(B, 64, 16, generator=torch.Generator().manual_seed(seed))


def test_refused_argument_combinations_name_the_argument():
    mel, wav = _mel(), torch.zeros(B, int(SECONDS * 16000))
    with pytest.raises(ValueError, match="strength"):
        make_pipeline()(**_args(strength=0.5))
    with pytest.raises(ValueError, match="init_audio and init_mel"):
        make_pipeline()(**_args(init_mel=mel, init_audio=wav, strength=0.5))
    with pytest.raises(ValueError, match="latents"):
        make_pipeline()(**_args(init_mel=mel, latents=torch.zeros(B, 8, 16, 4), strength=0.5))
    with pytest.raises(ValueError, match="init_mel"):
        make_pipeline()(**_args(init_mel=mel[:, :32], strength=0.5))
    with pytest.raises(ValueError, match="init_mel"):
        make_pipeline()(**_args(init_mel=mel[:2], strength=0.5))
    with pytest.raises(ValueError, match="init_audio"):
        make_pipeline()(**_args(init_audio=wav[:, :100], strength=0.5))
    with pytest.raises(ValueError, match="vae_encoder"):
        make_pipeline(encoder=False)(**_args(init_mel=mel, strength=0.5))
    with pytest.raises(ValueError, match="init_posterior"):
        make_pipeline()(**_args(init_mel=mel, strength=0.5, init_posterior="mean"))
    with pytest.raises(ValueError, match="strength"):
        make_pipeline()(**_args(init_mel=mel, strength=0.01))                   # int(12 * 0.01) == 0 steps


def test_no_init_is_the_present_path():
    """Without an init the call makes the stub calls it made before: N scheduler steps from `prepare_latents`' draw, no encoder call,
    no add_noise -- and `strength=1.0, init_mel=None` spelled out is the same call."""
    from tests.stubs import make_pipeline as old_pipeline
    a, b, old = make_pipeline(), make_pipeline(), old_pipeline()
    ra = a(**_args()).audios
    rb = b(**_args(strength=1.0, init_mel=None, init_audio=None)).audios
    ro = old(**_args()).audios
    assert np.array_equal(ra, rb) and np.array_equal(ra, ro)
    for p in (a, b):
        assert p.vae_encoder.calls == 0 and not hasattr(p.scheduler, "noised_at")
        assert p.scheduler.calls == old.scheduler.calls == N
        assert torch.equal(p.scheduler.first_samples[0], old.scheduler.first_samples[0])


def test_warm_start_runs_n_run_steps_from_the_noised_encoding():
    pipe = make_pipeline()
    mel = _mel()
    out = pipe(**_args(init_mel=mel, strength=0.5, output_type="latent")).audios
    s = pipe.scheduler
    full = list(s._timesteps_host)
    assert s.calls == N // 2 == len(pipe.last_losses) and pipe.vae_encoder.calls == 1
    assert s.noised_at == [full[N // 2]] and s.num_inference_steps == N
    assert torch.equal(pipe.vae_encoder.seen[0], mel)
    # the hand-written loop: per clip the posterior draw first, then the latent noise, from that clip's generator
    from diffmusic_amd.torch_utils import randn_tensor
    ref = make_pipeline()
    ref.scheduler.set_timesteps(N)
    gens = [torch.Generator().manual_seed(k) for k in range(B)]
    z0 = StubDist(mel).sample(gens) * StubVae.config.scaling_factor
    x = ref.scheduler.add_noise(z0, randn_tensor(z0.shape, generator=gens, dtype=torch.float32), full[N // 2])
    pe = ref._prepare_cond(_args()["prompt_embeds"], None, 1, True, "cpu")
    for t in full[N // 2:]:
        x = ref.scheduler.step(ref._unet_eps(x, t, pe, 2.0, True), t, x, eta=0.0).prev_sample
    assert torch.equal(out, x)
    # mode: no posterior draw, so the first draw of each generator is the latent noise
    m = make_pipeline()(**_args(init_mel=mel, strength=0.5, output_type="latent", init_posterior="mode")).audios
    gens = [torch.Generator().manual_seed(k) for k in range(B)]
    z0 = StubDist(mel).mode() * StubVae.config.scaling_factor
    x = ref.scheduler.add_noise(z0, randn_tensor(z0.shape, generator=gens, dtype=torch.float32), full[N // 2])
    for t in full[N // 2:]:
        x = ref.scheduler.step(ref._unet_eps(x, t, pe, 2.0, True), t, x, eta=0.0).prev_sample
    assert torch.equal(m, x) and not torch.equal(m, out)


def test_nan_retry_and_outer_iterations_encode_once():
    """A NaN at the third step restarts from a fresh noising of the SAME z0 (latent noise redrawn, nothing re-encoded); every outer
    iteration starts from the noised latent again."""
    pipe = make_pipeline(nan_at={2})
    pipe(**_args(init_mel=_mel(), strength=0.5))
    s = pipe.scheduler
    assert pipe.nan_restarts == 1 and pipe.vae_encoder.calls == 1
    assert s.calls == 3 + N // 2 and len(s.noised_at) == 2 and s.noised_at[0] == s.noised_at[1]
    two = make_pipeline()
    two(**_args(init_mel=_mel(), strength=0.5, optim_outer_loop=2))
    assert two.vae_encoder.calls == 1 and two.scheduler.calls == 2 * (N // 2) and len(two.scheduler.noised_at) == 1


def test_lanes_and_clip_order_do_not_change_a_warm_started_clip():
    """Per-clip draws and an encode of the clip's own rows: `lanes=2` equals `lanes=1`, and clip k equals a call on clip k alone."""
    mel = _mel()
    whole = make_pipeline()(**_args(init_mel=mel, strength=0.5, output_type="latent")).audios
    laned = make_pipeline()(**_args(init_mel=mel, strength=0.5, output_type="latent", lanes=2)).audios
    assert torch.equal(whole, laned)
    pe = _args()["prompt_embeds"]
    for k in range(B):
        one = make_pipeline()(**_args(init_mel=mel[k:k + 1], strength=0.5, output_type="latent", prompt_embeds=pe[k:k + 1],
                                      generator=[torch.Generator().manual_seed(k)])).audios
        assert torch.equal(one[0], whole[k])
