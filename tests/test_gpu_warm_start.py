"""-m gpu: warm-started sampling (`init_mel` / `init_audio` + `strength`) through the real pipeline on small networks (as in
tests/test_gpu_step.py) and once at full size: the call equals a hand-written loop bit for bit, the start latent matches the fp32
restatement, the cold path is untouched and launches no encoder op, a lane equals the call on its clips, and the measurement-noise
keys of a timestep are those of a cold run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HIFI = dict(model_in_dim=64, upsample_initial_channel=128, upsample_rates=[5, 4, 2, 2, 2], upsample_kernel_sizes=[16, 16, 8, 4, 4],
            resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, leaky_relu_slope=0.1, sampling_rate=16000)
VAE = dict(latent_channels=8, out_channels=1, block_out_channels=[32, 64, 64], layers_per_block=2, norm_num_groups=32,
           scaling_factor=0.9227914214134216, eps=1e-6)
UNET = dict(in_channels=8, out_channels=8, block_out_channels=[32, 64, 96, 160], layers_per_block=2, attention_heads=4,
            norm_num_groups=32, down_attn=[0, 1, 1, 1], up_attn=[1, 1, 1, 0], class_embed_dim=512)
SCHED = dict(num_train_timesteps=1000, beta_start=0.0015, beta_end=0.0195, beta_schedule="scaled_linear", clip_sample=False,
             set_alpha_to_one=False, steps_offset=1, prediction_type="epsilon", timestep_spacing="leading")
SECONDS, LEN, HEIGHT, B, N = 0.4, 6400, 40, 3, 20          # mel (B, 40, 64) -> latent (B, 8, 10, 16)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _pipe(sigma=0.0, stream="global", full=False):
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.pipelines import MusicLDMPipeline
    from diffmusic_amd.schedulers import get_scheduler
    if full:
        pipe = MusicLDMPipeline.from_pretrained("synthetic", seed=0)
    else:
        pipe = MusicLDMPipeline.from_pretrained("synthetic", seed=0, unet_config=UNET, vae_config=VAE, vocoder_config=HIFI)
    length = 160000 if full else LEN
    op = P.MusicInpaintingOperator(1, length, "box", 0.25, 0.5, 0.3, 0.1, 0.2, noiser=P.GaussianNoise(sigma, stream=stream))
    pipe.scheduler = get_scheduler("dps")(operator=op, **SCHED)
    pipe.assume_uncond_equals_cond = True
    return pipe, op


def _inputs(length=LEN, height=HEIGHT, seed=11):
    g = torch.Generator().manual_seed(seed)
    pe = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    mel = 2.0 * torch.randn(B, height, 64, generator=g) - 4.0
    clean = 0.3 * torch.sin(torch.arange(length) * 0.05)[None].repeat(B, 1) + 0.05 * torch.randn(B, length, generator=g)
    return pe, mel, clean


def _gens():
    return [torch.Generator().manual_seed(100 + k) for k in range(B)]


def _call(pipe, pe, y, **kw):
    args = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N, generator=_gens(), show_progress=False,
                measurement=y, output_type="latent", eta=0.0)
    args.update(kw)
    return pipe(**args).audios


def test_warm_call_equals_the_hand_written_loop():
    """encode -> posterior draw, then latent noise, per clip -> add_noise at timesteps[10] -> ten guided steps."""
    from diffmusic_amd.torch_utils import randn_tensor
    pipe, op = _pipe()
    pe, mel, clean = _inputs()
    y = op.forward(clean.cuda())
    out = _call(pipe, pe, y, init_mel=mel, strength=0.5)
    assert len(pipe.last_losses) == 10 and pipe.nan_restarts == 0
    s = pipe.scheduler
    s.set_timesteps(N, device="cuda")
    ts = list(s._timesteps_host)
    assert s.timesteps_for_strength(0.5) == ts[10:]
    gens = _gens()
    z0 = pipe.vae_encoder.encode(mel.cuda()).latent_dist.sample(gens)
    noise = randn_tensor(z0.shape, generator=gens, device=torch.device("cuda"), dtype=torch.float32)
    x = s.add_noise(z0 * pipe.vae.config.scaling_factor, noise, ts[10])
    cond = pipe._prepare_cond(pe, None, 1, True, torch.device("cuda"))
    for t in ts[10:]:
        eps = pipe._unet_eps(x, t, cond, 2.0, True)
        x = s.step(eps, t, x, eta=0.0, generator=gens, measurement=y, vae=pipe.vae, vocoder=pipe.vocoder, original_waveform_length=LEN,
                   ip_guidance_rate=5e-4, supervised_space="mel_spectrogram").prev_sample
    assert torch.equal(out, x)
    # the posterior mode makes no draw: another start, same number of steps
    m = _call(pipe, pe, y, init_mel=mel, strength=0.5, init_posterior="mode")
    assert len(pipe.last_losses) == 10 and not torch.equal(m, out)


def test_start_latent_against_the_fp32_restatement():
    from diffmusic_amd.torch_utils import randn_tensor
    from tests.test_gpu_vae_encoder import RefEncoder
    pipe, _ = _pipe()
    _, mel, _ = _inputs()
    enc = pipe.vae_encoder
    ref = RefEncoder(**enc.cfg).eval()
    ref.load_state_dict(enc.synth_state_dict(seed=3), strict=True)           # from_pretrained("synthetic", seed=0): encoder seed 3
    s = pipe.scheduler
    s.set_timesteps(N)
    t = s._timesteps_host[10]
    gens = _gens()
    z0 = enc.encode(mel.cuda()).latent_dist.sample(gens)
    noise = randn_tensor(z0.shape, generator=gens, device=torch.device("cuda"), dtype=torch.float32)
    got = s.add_noise(z0 * enc.scaling_factor, noise, t)
    gens = _gens()
    eps = randn_tensor(z0.shape, generator=gens, dtype=torch.float32)
    with torch.no_grad():
        mom = ref(mel).reshape(B, 10, 16, 16).permute(0, 3, 1, 2)
    sa, s1 = s.add_noise_scalars(t)
    want = sa * enc.scaling_factor * (mom[:, :8] + torch.exp(0.5 * mom[:, 8:].clamp(-30.0, 20.0)) * eps) + s1 * noise.cpu()
    r = _rel(got, want)
    print(f"warm-start latent rel-L2 vs fp32 restatement: {r:.3e}")
    assert r < 1e-2


def test_cold_path_is_untouched_and_launches_no_encoder_op(monkeypatch):
    from diffmusic_amd import ops
    pipe, op = _pipe()
    pe, mel, clean = _inputs()
    y = op.forward(clean.cuda())
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(hip, name)
            if name in ("vae_enc_fwd", "latent_init"):
                calls.append(name)
            return fn
    hip = ops.hip
    monkeypatch.setattr(ops, "hip", Counting())
    a = _call(pipe, pe, y)
    b = _call(pipe, pe, y, strength=1.0, init_mel=None, init_audio=None)
    assert torch.equal(a, b) and calls == [] and len(pipe.last_losses) == N
    _call(pipe, pe, y, init_mel=mel, strength=0.5)
    assert calls.count("vae_enc_fwd") == 1                                  # once per call, and the counter does see it


def test_measurement_noise_keys_are_those_of_a_cold_run():
    """With the per-clip measurement-noise stream the step index that keys the noise at a timestep is its position in the FULL list,
    warm or cold: the same (seed, step) and so the same (key, offset) of `clip_noise_key`."""
    pipe, op = _pipe(sigma=0.05, stream="clip")
    pe, mel, clean = _inputs()
    y = op.forward(clean.cuda())
    seen = []
    draw = op.noiser.draw

    def recording(shape, device, step=None, generator=None):
        seen.append((step, tuple(int(g.initial_seed()) for g in generator)))
        return draw(shape, device, step=step, generator=generator)
    op.noiser.draw = recording
    _call(pipe, pe, y, init_mel=mel, strength=0.5)
    warm = list(seen)
    del seen[:]
    _call(pipe, pe, y)
    cold = list(seen)
    seeds = tuple(100 + k for k in range(B))
    assert [s for s, _ in cold] == list(range(N)) and [s for s, _ in warm] == list(range(10, N))
    assert all(g == seeds for _, g in cold + warm)
    assert warm == cold[10:]
    # the lane loop builds its step keywords per lane: every lane draws with its own clips' seeds at the same full-list step indices
    del seen[:]
    _call(pipe, pe, y, init_mel=mel, strength=0.5, lanes=2)
    assert sorted(set(s for s, _ in seen)) == list(range(10, N))
    for step in range(10, N):
        assert sorted(k for s, g in seen if s == step for k in g) == list(seeds)


def _lane_problem():
    pipe, op = _pipe(sigma=0.05, stream="clip")
    pe, mel, clean = _inputs()
    return pipe, pe, mel, op.forward(clean.cuda())


def test_a_lane_of_a_warm_call_is_the_warm_call_on_its_clips():
    """The property tests/test_gpu_lanes.py holds for the cold path, with an init: bit for bit (the encode and the per-clip draws do not
    depend on the clips around a clip)."""
    from diffmusic_amd.pipelines.lanes import split_sizes
    pipe, pe, mel, y = _lane_problem()
    two = _call(pipe, pe, y, init_mel=mel, strength=0.5, lanes=2)
    o = 0
    for n in split_sizes(B, 2):
        ids = list(range(o, o + n))
        part = pipe(prompt_embeds=pe[ids], audio_length_in_s=SECONDS, num_inference_steps=N, show_progress=False, eta=0.0,
                    generator=[torch.Generator().manual_seed(100 + k) for k in ids], measurement=y[ids].contiguous(),
                    output_type="latent", init_mel=mel[ids], strength=0.5).audios
        assert torch.equal(two[ids], part), f"lane {ids} differs from the warm-started call on those clips"
        o += n


def test_lanes2_equals_lanes1_with_an_init():
    """`lanes=2` against `lanes=1` on the same 3-clip batch, bit for bit, with an init and on the cold path: the encode and the draws
    happen once before the split, and no kernel plan of the guided step may depend on the batch (the GroupNorm plan once did: a
    1-clip lane's CFG batch of 2 fell below its `B * G >= 128` threshold and took another plan than the 3-clip batch)."""
    pipe, pe, mel, y = _lane_problem()
    one = _call(pipe, pe, y, init_mel=mel, strength=0.5, lanes=1)
    two = _call(pipe, pe, y, init_mel=mel, strength=0.5, lanes=2)
    cold1, cold2 = _call(pipe, pe, y, lanes=1), _call(pipe, pe, y, lanes=2)
    print(f"lanes=2 vs lanes=1 rel-L2 of the final latents: warm {_rel(two, one):.3e}, cold {_rel(cold2, cold1):.3e}")
    assert torch.equal(one, two)
    assert torch.equal(cold1, cold2)


def test_full_size_init_audio_runs_the_kept_steps():
    """Headline architecture, 10 s clips: `init_audio` (the measurement itself) through ModelMelFrontend and the encoder, strength 0.3 of
    10 steps = 3 guided steps, finite result."""
    pipe, op = _pipe(full=True)
    pe, _, clean = _inputs(length=160000, height=1000)
    y = op.forward(clean.cuda())
    out = pipe(prompt_embeds=pe, audio_length_in_s=10.0, num_inference_steps=10, generator=_gens(), show_progress=False, measurement=y,
               output_type="latent", init_audio=y, strength=0.3).audios
    assert out.shape == (B, 8, 250, 16) and len(pipe.last_losses) == 3 and bool(torch.isfinite(out).all())
