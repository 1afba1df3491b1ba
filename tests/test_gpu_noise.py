"""-m gpu: measurement noise (sigma > 0) inside every guided step.  The reference's operators end `forward` in `self.noiser(...)`
(diffmusic/inverse_problem/operator.py:132-133, 170-171, 203-205, 247-250, 270-271) and its schedulers call `forward` on the predicted
audio in every step (scheduling_dps.py:200 and siblings), so with sigma > 0 the loss is taken on A(wav) + sigma * z.

Covered: the fused STFT -> mel -> loss kernels with a sample-domain / magnitude-domain additive input against float64 torch
(the cases and bounds of tests/test_gpu_stft_mel.py), an all-zero additive input as a bitwise no-op, fused route = composed route per
operator, teacher-forced guided steps against the CPU oracle with the same injected draw (bounds of tests/test_gpu_step.py), the
per-clip stream (its documented key; batch, lane and split independence), a production-size N = 10 trajectory against the oracle
loop, both bindings of the new ops, and sigma = 0 changing nothing."""
import math
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
from tests.test_gpu_stft_mel import CASES as STFT_CASES, _clips                     # noqa: E402
from tests.test_gpu_step import HIFI, VAE, SCHED, H, W, LEN                        # noqa: E402

_NEG, _POS = -3.0e38, 3.0e38


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-300))


# ---- 1 / 2: kernel level ---------------------------------------------------------------------------------------------------------
def _truth(wav, mask, fb, ref, L, hop, hann, power2, to_db, lo, hi, add=None, addmag=None):
    """tests/test_gpu_stft_mel.py::_truth with the additive inputs: float64 torch (mel (B, T, 64), loss (B), dwav (B, full))."""
    w = wav.double().clone().requires_grad_(True)
    y = w[:, :L] * (mask.double() if mask is not None else 1.0)
    if add is not None:
        y = y + add.double()[:, :L]
    win = torch.hann_window(1024, periodic=True, dtype=torch.float64, device=wav.device) if hann else torch.ones(1024, dtype=torch.float64, device=wav.device)
    spec = torch.stft(y, 1024, hop, 1024, window=win, center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    p = spec.real ** 2 + spec.imag ** 2
    if not power2:
        p = torch.sqrt(p)
        if addmag is not None:
            p = p + addmag.double()
    mel_lin = torch.einsum("bkt,km->btm", p, fb.double())
    mel = 10.0 * torch.log10(torch.clamp(mel_lin, min=1e-10)) if to_db else mel_lin
    mel = torch.clamp(mel, lo, hi)
    loss = torch.linalg.vector_norm((ref.double() - mel).flatten(1), dim=1)
    (g,) = torch.autograd.grad(loss.sum(), w)
    return mel.detach(), loss.detach(), g


def _kernel_problem(case):
    from diffmusic_amd.inverse_problem.operator import SpectralFrontend
    name, L, full, hop, hann, power2, to_db, lo, hi, masked, shared = case
    B = 3
    fe = SpectralFrontend(16000, 1024, hop, 64, "hann" if hann else "rect")
    assert fe.fused(L)
    wav = _clips(B, full, 1)
    mask = None
    if masked:
        mask = torch.ones(L)
        mask[L // 5: L // 5 + L // 10] = 0.0
        mask[:300] = 0.0
        mask = mask.cuda()
    target = _clips(1 if shared else B, L, 2)
    ref = fe.transform_fwd(target, L, power2, to_db, lo, hi).clone()
    g = torch.Generator().manual_seed(11)
    if power2:                                             # sample domain; `ragged_length` hands a (B, full) tensor: row stride != L
        z = torch.randn(B, full if name == "ragged_length" else L, generator=g).cuda()
        kw, sigma = dict(noise=z), 0.05
    else:                                                  # magnitude domain (phase retrieval): rectangular-window magnitudes are in the hundreds
        z = torch.randn(B, 513, 1 + L // hop, generator=g).cuda()
        kw, sigma = dict(noise_mag=z), 8.0
    return fe, wav, mask, ref, kw, sigma, B


@pytest.mark.parametrize("case", STFT_CASES, ids=[c[0] for c in STFT_CASES])
def test_fused_guidance_with_additive_input_matches_float64_torch(case):
    from diffmusic_amd.inverse_problem import dsp
    name, L, full, hop, hann, power2, to_db, lo, hi, masked, shared = case
    fe, wav, mask, ref, kw, sigma, B = _kernel_problem(case)
    fb = torch.from_numpy(dsp.melscale_fbanks(513, 0.0, 8000.0, 64, 16000)).cuda()
    add = sigma * kw["noise"].double() if "noise" in kw else None
    addmag = sigma * kw["noise_mag"].double() if "noise_mag" in kw else None
    _, loss_t, g_t = _truth(wav, mask, fb, ref, L, hop, hann, power2, to_db, max(lo, -1e300), min(hi, 1e300), add, addmag)
    _, loss_0, _ = _truth(wav, mask, fb, ref, L, hop, hann, power2, to_db, max(lo, -1e300), min(hi, 1e300))
    assert float(((loss_t - loss_0).abs() / loss_0).min()) > 1e-3, (name, loss_t, loss_0)        # the additive input matters in this case
    loss, dwav = fe.guidance(wav, L, ref, mask, power2, to_db, lo, hi, sigma=sigma, **kw)
    assert loss.shape == (B,) and dwav.shape == (B, full)
    rl = float(((loss.double() - loss_t).abs() / loss_t).max())
    rg, r0, r1 = _rel(dwav[:, :L], g_t[:, :L]), _rel(dwav[:, :600], g_t[:, :600]), _rel(dwav[:, L - 600:L], g_t[:, L - 600:L])
    print(f"\n  {name}: loss {rl:.2e} grad {rg:.2e} first600 {r0:.2e} last600 {r1:.2e}")
    assert rl < 2e-5, (name, loss, loss_t)
    assert rg < 2e-4, (name, rg)
    assert r0 < 5e-4 and r1 < 5e-4, (name, r0, r1)
    if full > L:
        assert float(dwav[:, L:].abs().max()) == 0.0
    if mask is not None:
        assert float(dwav[:, :L][:, mask == 0].abs().max()) == 0.0                 # masked samples: the noise has no gradient path
    loss2, dwav2 = fe.guidance(wav, L, ref, mask, power2, to_db, lo, hi, sigma=sigma, **kw)
    assert torch.equal(loss, loss2) and torch.equal(dwav, dwav2)


@pytest.mark.parametrize("case", STFT_CASES, ids=[c[0] for c in STFT_CASES])
def test_additive_input_of_zeros_is_a_bitwise_noop(case):
    name, L, full, hop, hann, power2, to_db, lo, hi, masked, shared = case
    fe, wav, mask, ref, kw, sigma, B = _kernel_problem(case)
    loss0, dwav0 = fe.guidance(wav, L, ref, mask, power2, to_db, lo, hi)
    zeros = {k: torch.zeros_like(v) for k, v in kw.items()}
    loss1, dwav1 = fe.guidance(wav, L, ref, mask, power2, to_db, lo, hi, sigma=sigma, **zeros)
    assert torch.equal(loss0, loss1) and torch.equal(dwav0, dwav1), name
    loss2, dwav2 = fe.guidance(wav, L, ref, mask, power2, to_db, lo, hi, sigma=0.0, **kw)      # and so is a zero scale
    assert torch.equal(loss0, loss2) and torch.equal(dwav0, dwav2), name


# ---- 3: fused route = composed route, per operator ---------------------------------------------------------------------------------
def test_operators_with_noise_match_their_composed_path():
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.inverse_problem import dsp
    from diffmusic_amd.inverse_problem.operator import l2_loss
    L, full = 32000, 32032
    wav = _clips(2, full, 5)
    clean = _clips(2, L, 6)
    g = torch.Generator().manual_seed(12)
    ops_ = ((P.MusicInpaintingOperator(2, 16000, "box", 0.5, 0.9, 0.3, 0.1, 0.2, noiser=P.GaussianNoise(0.05)), (2, L)),
            (P.SuperResolutionOperator(16000, 2, noiser=P.GaussianNoise(0.05)), (2, L // 2)),
            (P.PhaseRetrievalOperator(noiser=P.GaussianNoise(8.0)), (2, 513, 1 + L // 160)))
    for op, shape in ops_:
        sigma = op.noiser.sigma
        z = torch.randn(shape, generator=g).cuda()
        quiet = op.noiser
        op.noiser = None
        meas = op.forward(clean)                              # a noiseless measurement: this test is about the step
        op.noiser = quiet
        loss, dwav = op.guidance(wav, L, meas, "mel_spectrogram", noise=z)
        fe = op.frontend
        if isinstance(op, P.PhaseRetrievalOperator):
            ref = fe.melscale(meas, -80.0, 80.0)
            pred = fe.melscale((fe.stft_mag(wav, L) + sigma * z).contiguous(), -80.0, 80.0)          # (B, T, 64)
            l2, dmel = l2_loss(ref, pred)
            fb = torch.from_numpy(dsp.melscale_fbanks(513, 0.0, 8000.0, 64, 16000)).cuda()
            inside = ((pred > -80.0) & (pred < 80.0)).float()
            dmag = torch.einsum("btm,km->bkt", dmel * inside, fb).contiguous()
            d2 = torch.zeros_like(wav)
            fe.stft_mag_bwd(dmag, L, d2)
        else:
            y, adj = op.apply(wav, L)
            y = (y + sigma * z).contiguous()
            ref = op._mel(meas).clone()
            pred = op._mel(y)
            l2, dmel = l2_loss(ref, pred)
            d2 = adj(fe.transform_bwd(dmel), full)
        rl, rg = float(((loss - l2).abs() / l2).max()), _rel(dwav, d2)
        print(f"\n  {type(op).__name__}: loss {rl:.2e} grad {rg:.2e}")
        assert rl < 1e-5, type(op).__name__
        assert rg < 1e-5, (type(op).__name__, rg)
        assert math.isfinite(float(dwav.abs().max()))
        quiet_loss, _ = op.guidance(wav, L, meas, "mel_spectrogram", noise=torch.zeros_like(z))
        assert float(((loss - quiet_loss).abs() / quiet_loss).min()) > 1e-3            # and the noise is really in there


def test_style_operator_noise_equals_a_noisy_input():
    """StyleGuidanceOperator.forward is noiser(identity): the step with noise z on wav is the noiseless step on wav + sigma * z, bit for
    bit (same kernels on the same values), in both supervised spaces; the gradient has no extra term."""
    import bench
    from diffmusic_amd import ops, inverse_problem as P
    L, sigma = 32000, 0.05
    y = torch.stack([bench.synth_clip(1, L), bench.synth_clip(2, L)]).cuda()
    g = torch.Generator().manual_seed(13)
    wav = torch.cat([0.5 * y + 0.05 * torch.randn(2, L, generator=g).cuda(), torch.zeros(2, 32, device="cuda")], dim=1).contiguous()
    z = torch.randn(2, L, generator=g).cuda()
    op = P.StyleGuidanceOperator(16000, noiser=P.GaussianNoise(sigma), device="cuda", seed=3)
    noisy_in = ops.hip.noise_add(wav[:, :L].contiguous(), z, sigma)
    for space in ("wav_form", "mel_spectrogram"):
        op.noiser = P.GaussianNoise(sigma)
        loss, dwav = op.guidance(wav, L, y, space, noise=z)
        assert dwav.shape == wav.shape and float(dwav[:, L:].abs().max()) == 0.0
        op.noiser = None
        loss_q, dwav_q = op.guidance(noisy_in, L, y, space)
        assert torch.equal(loss, loss_q) and torch.equal(dwav[:, :L], dwav_q), space
        loss_0, _ = op.guidance(wav, L, y, space)
        assert not torch.equal(loss, loss_0), space


# ---- 4: teacher-forced guided step against the oracle -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    from diffmusic_amd.engine import HifiGanEngine, VaeDecoderEngine
    from oracle.models import HifiGan, VaeDecoder
    voc, vae = HifiGanEngine(HIFI), VaeDecoderEngine(VAE)
    sv, sa = voc.synth_state_dict(seed=1), vae.synth_state_dict(seed=2)
    voc.load_state_dict(sv)
    vae.load_state_dict(sa)
    rvoc, rvae = HifiGan(**HIFI), VaeDecoder(**VAE)
    rvoc.load_state_dict(sv, strict=False)
    rvae.load_state_dict(sa, strict=True)
    return voc, vae, rvoc.eval(), rvae.eval()


class _FixedNoiser:
    """Oracle-side noiser: data + sigma * z with a given draw (the oracle's operators call whatever callable they are given)."""

    def __init__(self, sigma, z):
        self.sigma, self.z = sigma, z

    def __call__(self, data):
        return data + self.sigma * self.z


def _noisy_ops(task, sigma):
    from diffmusic_amd import inverse_problem as P
    from oracle import operators as O
    n = P.GaussianNoise(sigma)
    if task == "music_inpainting":
        args = (1, LEN, "box", 0.25, 0.5, 0.3, 0.1, 0.2)
        return P.MusicInpaintingOperator(*args, noiser=n), O.MusicInpaintingOperator(*args), (LEN,)
    if task == "phase_retrieval":
        return P.PhaseRetrievalOperator(noiser=n), O.PhaseRetrievalOperator(), (513, 1 + LEN // 160)
    if task == "super_resolution":
        return P.SuperResolutionOperator(16000, 2, noiser=n), O.SuperResolutionOperator(16000, 2), (LEN // 2,)
    if task == "super_resolution4":
        return P.SuperResolutionOperator(16000, 4, noiser=n), O.SuperResolutionOperator(16000, 4), (LEN // 4,)
    assert task == "music_dereverberation"
    return P.MusicDereverberationOperator(500, 0.99, noiser=n), O.MusicDereverberationOperator(500, 0.99), (LEN + 1,)


# sigma per case: the smallest of 0.05 / 0.5 / 8.0 (the sizes at which a stand-in prediction moves the loss by 11-28 %) and their
# multiples at which the ORACLE's loss on the toy networks moves by more than 5e-2 (asserted below).  On these untrained networks the
# prediction is far from the measurement, so the noise term sigma^2 * n competes with a large ||y - A(x)||^2: super-resolution and
# wav_form inpainting at 0.05 moved the oracle's loss by 0.2-0.5 %, phase retrieval at 8.0 by 3-4 %, hence the larger values there.
NOISY_CASES = [("dps", "music_inpainting", 0.0, 5e-4, "mel_spectrogram", 501, 0.05, True),
               ("dps", "music_inpainting", 0.0, 5e-4, "wav_form", 996, 0.5, True),
               ("mpgd", "super_resolution4", 0.0, 5e-3, "mel_spectrogram", 501, 0.3, True),
               ("dps", "super_resolution", 0.0, 5e-4, "wav_form", 251, 0.5, True),
               ("dps", "music_dereverberation", 0.0, 5e-4, "mel_spectrogram", 501, 0.5, True),
               ("dsg", "phase_retrieval", 1.0, 0.08, "mel_spectrogram", 501, 16.0, True),
               ("dps", "phase_retrieval", 0.0, 5e-4, "wav_form", 501, 16.0, True),
               ("dps", "music_inpainting", 0.0, 5e-4, "mel_spectrogram", 501, 0.05, False)]


@pytest.mark.parametrize("name,task,eta,rate,space,t,sigma,per_clip", NOISY_CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[4]}-{'clip' if c[7] else 'batch'}" for c in NOISY_CASES])
def test_teacher_forced_noisy_step(nets, name, task, eta, rate, space, t, sigma, per_clip):
    """`_teacher_forced` of tests/test_gpu_step.py with the step's noise injected on both sides: `op_kwargs=dict(noise=z)` for the
    product, a noiser returning data + sigma * z for the oracle.  Same bounds: prev rel-L2 < 1e-2, loss < 1e-2, gradient cosine > 0.98.
    Before that, on the oracle alone: the loss with the step noise and the loss without it differ by more than 5e-2 relative, so a
    product that ignored the noise could not pass the loss bound."""
    from diffmusic_amd.schedulers import get_scheduler
    from oracle import schedulers as OS
    voc, vae, rvoc, rvae = nets
    op, rop, zshape = _noisy_ops(task, sigma)
    B = 2
    g = torch.Generator().manual_seed(77)
    clean = 0.3 * torch.sin(torch.arange(LEN) * 0.05)[None] * torch.tensor([[1.0], [0.6]]) + 0.05 * torch.randn(B, LEN, generator=g)
    opk = {}
    if task == "music_dereverberation":       # pin the impulse response (the reference redraws it on every call)
        opk = dict(ir=rop.generate_impulse_response(500, 0.99))
    x = torch.randn(B, 8, H, W, generator=g)
    e = torch.randn(B, 8, H, W, generator=g)
    zs = torch.randn(B, 8, H, W, generator=g)
    z_meas = torch.randn((B,) + zshape, generator=g)          # the measurement's own draw, made once by the oracle
    z = torch.randn((B,) + zshape, generator=g)               # the step's draw, shared by both sides
    rop.noiser = _FixedNoiser(sigma, z_meas)
    y_ref = rop.forward(clean, **opk)
    assert tuple(y_ref.shape) == (B,) + zshape
    y = y_ref.cuda()
    kw = dict(eta=eta, ip_guidance_rate=rate, original_waveform_length=LEN, supervised_space=space)
    rnoise = dict(sample_noise=zs) if name in ("dsg", "diffmusic") else dict(variance_noise=zs if eta > 0 else None)

    def oracle_step(noiser):
        rop.noiser = noiser
        rs = OS.get_scheduler(name)(operator=rop, per_clip_norm=per_clip, **SCHED)
        rs.set_timesteps(200)
        return rs.step(e, t, x, measurement=y_ref, vae=rvae, vocoder=rvoc, op_kwargs=opk, **kw, **rnoise)

    ro = oracle_step(_FixedNoiser(sigma, z))
    quiet = oracle_step(_FixedNoiser(0.0, z))
    gap = float(((ro.loss.reshape(-1) - quiet.loss.reshape(-1)).abs() / quiet.loss.reshape(-1).abs()).min())
    msg = f"{name}/{task}/{space}/sigma={sigma}: oracle loss with vs without the step noise {gap:.3f}"
    print("\n  " + msg)
    assert gap > 5e-2, msg

    sched = get_scheduler(name)(operator=op, per_clip_norm=per_clip, **SCHED)
    sched.set_timesteps(200)
    sched.debug_keep_grad = True
    noise_kw = dict(sample_noise=zs.cuda()) if name in ("dsg", "diffmusic") else dict(variance_noise=zs.cuda() if eta > 0 else None)
    out = sched.step(e.cuda(), t, x.cuda(), measurement=y, vae=vae, vocoder=voc, op_kwargs=dict(opk, noise=z.cuda()), **kw, **noise_kw)
    torch.cuda.synchronize()
    rp = _rel(out.prev_sample, ro.prev_sample)
    rl = _rel(out.loss.reshape(-1), ro.loss.reshape(-1))
    rg = _rel(sched.last_grad, ro.sample)
    cos = torch.nn.functional.cosine_similarity(sched.last_grad.cpu().flatten(), ro.sample.flatten(), dim=0).item()
    msg += f"; prev {rp:.2e} loss {rl:.2e} grad {rg:.2e} cos {cos:.4f}"
    print("  " + msg)
    assert _rel(out.pred_original_sample, ro.pred_original_sample) < 1e-4 or name == "mpgd"
    assert rl < 1e-2, msg
    assert cos > 0.98, msg
    assert rp < 1e-2, msg


# ---- 5: the per-clip stream ---------------------------------------------------------------------------------------------------------
def _clip_ops():
    from diffmusic_amd import inverse_problem as P
    L = 32000
    return ((P.MusicInpaintingOperator(2, 16000, "box", 0.5, 0.9, 0.3, 0.1, 0.2, noiser=P.GaussianNoise(0.05, stream="clip")), (L,), "mel_spectrogram"),
            (P.SuperResolutionOperator(16000, 2, noiser=P.GaussianNoise(0.05, stream="clip")), (L // 2,), "wav_form"),
            (P.PhaseRetrievalOperator(noiser=P.GaussianNoise(8.0, stream="clip")), (513, 1 + L // 160), "mel_spectrogram")), L


def test_clip_stream_draw_is_randn_philox_under_the_documented_key():
    from diffmusic_amd import ops
    from diffmusic_amd.inverse_problem.noise import MEASUREMENT_KEY_XOR, clip_noise_key
    from diffmusic_amd.torch_utils import randn_philox
    opsl, L = _clip_ops()
    B, step, seeds = 3, 4, [100, 101, (1 << 63) + 9]
    wav, clean = _clips(B, L + 32, 5), _clips(B, L, 6)
    for op, zshape, space in opsl:
        noiser, op.noiser = op.noiser, None
        meas = op.forward(clean)
        op.noiser = noiser
        gens = [torch.Generator().manual_seed(s) for s in seeds]
        loss, dwav = op.guidance(wav, L, meas, space, step=step, generator=gens)
        keys = [(s ^ MEASUREMENT_KEY_XOR) & 0xFFFFFFFFFFFFFFFF for s in seeds]                # the key, spelled out
        z = randn_philox((B,) + zshape, keys, step << 32, "cuda")
        assert [clip_noise_key(s, step) for s in seeds] == [(k - (1 << 64) if k >= 1 << 63 else k, step << 32) for k in keys]
        assert torch.equal(z, ops.load().randn_philox([B] + list(zshape), [clip_noise_key(s, step)[0] for s in seeds], step << 32, torch.device("cuda")))
        loss_z, dwav_z = op.guidance(wav, L, meas, space, noise=z)
        assert torch.equal(loss, loss_z) and torch.equal(dwav, dwav_z), type(op).__name__
        # disjoint from the sampler stream of the same generators (device_noise=True draws under key = seed)
        assert not torch.equal(z, randn_philox((B,) + zshape, seeds, step << 32, "cuda"))
        assert abs(float(z.mean())) < 0.02 and abs(float(z.std()) - 1.0) < 0.02
        # another step, other noise
        loss_n, _ = op.guidance(wav, L, meas, space, step=step + 1, generator=gens)
        assert not torch.equal(loss, loss_n)


def test_clip_stream_batch_of_four_equals_two_batches_of_two():
    opsl, L = _clip_ops()
    wav, clean = _clips(4, L + 32, 7), _clips(4, L, 8)
    for op, zshape, space in opsl:
        noiser, op.noiser = op.noiser, None
        meas = op.forward(clean)
        op.noiser = noiser
        gens = [torch.Generator().manual_seed(40 + k) for k in range(4)]
        loss, dwav = op.guidance(wav, L, meas, space, step=2, generator=gens)
        for ids in ([0, 1], [2, 3]):
            l2, d2 = op.guidance(wav[ids].contiguous(), L, meas[ids].contiguous(), space, step=2, generator=[gens[k] for k in ids])
            assert torch.equal(loss[ids], l2) and torch.equal(dwav[ids], d2), (type(op).__name__, ids)


def _lane_problem(B, noiser, seed=3):
    from diffmusic_amd import inverse_problem as P
    from tests.test_gpu_pipeline import UNET, _build
    L = 6400
    op = P.MusicInpaintingOperator(1, L, "box", 0.25, 0.5, 0.3, 0.1, 0.2, noiser=noiser)
    pipe = _build("musicldm", UNET, "dps", op)
    g = torch.Generator().manual_seed(seed)
    clean = 0.3 * torch.sin(torch.arange(L) * 0.05)[None].repeat(B, 1) + 0.05 * torch.randn(B, L, generator=g)
    y = (clean * op.mask).cuda()
    pe = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    lat0 = torch.randn(B, 8, 10, 16, generator=g)
    return pipe, y, pe, ne, lat0


def _lane_call(pipe, y, pe, ne, lat0, ids, N, lanes):
    gens = [torch.Generator().manual_seed(100 + k) for k in ids]
    out = pipe(prompt_embeds=pe[ids], negative_prompt_embeds=ne[ids], audio_length_in_s=0.4, num_inference_steps=N, guidance_scale=2.0,
               latents=lat0[ids].clone(), measurement=y[ids].contiguous(), ip_guidance_rate=5e-4, eta=0.0, generator=gens,
               show_progress=False, output_type="latent", lanes=lanes)
    return out.audios, [l.reshape(-1).clone() for l in pipe.last_losses]


def test_clip_stream_lanes_equal_the_clip_groups_run_alone():
    """tests/test_gpu_lanes.py with sigma > 0 on the per-clip stream: the noise a clip sees does not depend on its lane."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.pipelines.lanes import split_sizes
    B, N, n_lanes = 4, 5, 2
    pipe, y, pe, ne, lat0 = _lane_problem(B, P.GaussianNoise(0.05, stream="clip"))
    got, losses = _lane_call(pipe, y, pe, ne, lat0, list(range(B)), N, n_lanes)
    assert got.shape == (B, 8, 10, 16) and len(losses) == N
    o = 0
    for n in split_sizes(B, n_lanes):
        ids = list(range(o, o + n))
        ref, ref_losses = _lane_call(pipe, y, pe, ne, lat0, ids, N, 1)
        assert torch.equal(got[ids], ref), f"lane {ids}: latents differ from the plain loop on those clips"
        for i in range(N):
            assert torch.equal(losses[i][ids], ref_losses[i]), f"lane {ids}: loss of step {i} differs"
        o += n
    whole, whole_losses = _lane_call(pipe, y, pe, ne, lat0, list(range(B)), N, 1)
    assert torch.equal(whole, got)                               # and the whole batch in the plain loop
    pipe.scheduler.operator.noiser = P.GaussianNoise(0.0)
    _, quiet = _lane_call(pipe, y, pe, ne, lat0, list(range(B)), N, 1)
    assert all(not torch.equal(a, b) for a, b in zip(whole_losses, quiet))      # the noise moves the loss from the first step on
    pipe.scheduler.operator.noiser = P.GaussianNoise(0.05)       # the process-wide stream is refused under lanes
    with pytest.raises(ValueError, match="per-clip noise stream"):
        _lane_call(pipe, y, pe, ne, lat0, list(range(B)), N, n_lanes)


def test_clip_stream_two_ranks_bit_equal_to_single_rank(tmp_path):
    """tests/test_gpu_multirank.py::test_pipeline_shard_two_ranks_bit_equal_to_single_rank with sigma > 0 on the per-clip stream: two rank
    processes on this GPU (gloo), `Pipeline.__call__(shard=True)`; every rank ends with all clips, bit-equal to the same clips run without
    torch.distributed in the per-rank batch compositions.  The noise a clip sees does not depend on the number of ranks."""
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n_clips = 5
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = str(tmp_path / "gathered.npy")
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(root, "tests", "noise_multirank_worker.py"), str(n_clips), out],
                                      env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=600)
            logs.append(o)
    finally:
        for p in procs:                      # exactly the processes started above
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-1500:] for l in logs)
    from tests.noise_multirank_worker import _quiet_problem, gens, problem
    pipe, kw = problem(n_clips)
    ref = np.zeros((n_clips, 6400), dtype=np.float32)
    for rank in range(2):
        sel = list(range(rank, n_clips, 2))
        kws = dict(kw, prompt_embeds=kw["prompt_embeds"][sel], measurement=kw["measurement"][sel].contiguous())
        ref[sel] = np.asarray(pipe(generator=[gens(n_clips)[k] for k in sel], **kws).audios)
    assert np.isfinite(ref).all() and float(np.abs(ref).max()) > 1e-3
    for rank in range(2):
        got = np.load(out.replace(".npy", f"_rank{rank}.npy"))
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), (rank, float(np.abs(got - ref).max()))
    qpipe, qkw = _quiet_problem(n_clips)                     # and the noise is really in the sharded run
    quiet = np.asarray(qpipe(generator=gens(n_clips), **qkw).audios)
    assert not np.array_equal(quiet, ref)


def test_global_stream_follows_torch_manual_seed():
    from diffmusic_amd import inverse_problem as P
    B, N = 2, 3
    pipe, y, pe, ne, lat0 = _lane_problem(B, P.GaussianNoise(0.05))
    runs = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        runs.append(_lane_call(pipe, y, pe, ne, lat0, list(range(B)), N, 1))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert not torch.equal(runs[0][1][0], runs[2][1][0])


# ---- 6: production-size short trajectory against the oracle loop --------------------------------------------------------------------
def test_fullsize_noisy_short_trajectory_snr():
    """The noisy twin of tests/test_gpu_batch_parity.py::test_fullsize_short_trajectory_snr: dps_inpainting, N = 10, one clip, sigma =
    0.05 on the per-clip stream.  The ten draws are reproduced with `randn_philox` under the documented key and handed to the oracle
    loop through a stateful noiser.  Same bars: waveform SNR >= 30 dB, every step's loss within 1e-2."""
    import bench
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.inverse_problem.noise import clip_noise_key
    from diffmusic_amd.torch_utils import randn_philox
    from oracle import schedulers as OS
    from tests.test_gpu_batch_parity import _dump, _rel as _rel64, _snr_db
    from tests.test_gpu_fullsize_parity import _oracle_nets, _oracle_op
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    dev = torch.device("cuda")
    wl, N, sigma, seed = "dps_inpainting", 10, 0.05, 0
    pname, sname, eta, rate, task, _, _ = bench.WORKLOADS[wl]
    pipe, op, meas, lat, cond, L = bench.build_problem(1, 0, dev, wl)
    pe = cond["class_labels"][:1]
    call = dict(prompt_embeds=pe, negative_prompt_embeds=pe, audio_length_in_s=bench.SECONDS, num_inference_steps=N,
                guidance_scale=bench.GUIDANCE_SCALE, measurement=meas, ip_guidance_rate=rate, eta=eta, show_progress=False)
    pipe(latents=lat.clone(), output_type="latent", generator=[torch.Generator().manual_seed(seed)], **call)
    quiet_losses = [float(l.reshape(-1)[0]) for l in pipe.last_losses]
    pipe.scheduler.operator = P.MusicInpaintingOperator(bench.SECONDS, bench.SR, "box", 2, 3, 0.3, 0.1, 1.0,
                                                        noiser=P.get_noiser("gaussian", sigma, stream="clip"))
    out = pipe(latents=lat.clone(), output_type="np", generator=[torch.Generator().manual_seed(seed)], **call)
    assert out.audios.shape == (1, L) and pipe.nan_restarts == 0
    hip_losses = [float(l.reshape(-1)[0]) for l in pipe.last_losses]
    assert all(a != b for a, b in zip(hip_losses, quiet_losses)), (hip_losses, quiet_losses)     # noisy from the first step on

    class Replay:                                             # oracle-side noiser: the product's ten draws, in step order
        def __init__(self):
            self.i = 0

        def __call__(self, data):
            key, off = clip_noise_key(seed, self.i)
            self.i += 1
            return data + sigma * randn_philox((1, L), [key], off, "cuda").cpu()

    ru, rv, rh = _oracle_nets(pipe, wl)
    rop = _oracle_op(task, op)
    yr = rop.forward(bench.synth_clip(0, L)[None])            # noiseless measurement, as build_problem made it
    rop.noiser = Replay()
    rs = OS.get_scheduler(sname)(operator=rop, **bench.SCHED_CFG)
    rs.set_timesteps(N)
    x, pec = lat.cpu().float(), pe.cpu()
    losses = []
    for t in [int(v) for v in rs.timesteps]:
        with torch.no_grad():
            e2 = ru(torch.cat([x, x]), t, class_labels=torch.cat([pec, pec]))[0]
        e = e2[:1] + bench.GUIDANCE_SCALE * (e2[1:] - e2[:1])
        so = rs.step(e, t, x, eta=eta, measurement=yr, vae=rv, vocoder=rh, original_waveform_length=L, ip_guidance_rate=rate,
                     supervised_space="mel_spectrogram")
        x = so.prev_sample.detach()
        losses.append(float(so.loss.reshape(-1)[0]))
    assert rop.noiser.i == N
    with torch.no_grad():
        wav = rh(rv.decode(x / rv.config.scaling_factor).sample.squeeze(1))[:, :L]
    snr = _snr_db(wav, torch.from_numpy(out.audios))
    lrel = max(abs(a - b) / abs(b) for a, b in zip(hip_losses, losses))
    print(f"\n  {wl} sigma={sigma} stream=clip: N={N} full-size waveform SNR vs oracle loop {snr:.1f} dB (noiseless twin: 53.7 dB); "
          f"worst per-step loss rel err {lrel:.2e}; first-step loss {hip_losses[0]:.2f} vs {quiet_losses[0]:.2f} at sigma 0")
    lat_hip = pipe(latents=lat.clone(), output_type="latent", generator=[torch.Generator().manual_seed(seed)], **call).audios
    _dump(f"trajectory_{wl}_sigma{sigma}.json",
          {"workload": wl, "steps": N, "sigma": sigma, "stream": "clip", "snr_db": snr, "loss_rel_worst": lrel,
           "final_latent_rel": _rel64(lat_hip, x), "oracle_losses": losses, "hip_losses": hip_losses, "hip_losses_sigma0": quiet_losses})
    assert snr >= 30.0
    assert lrel < 1e-2


# ---- 7: both bindings ---------------------------------------------------------------------------------------------------------------
def test_new_ops_equal_ctypes_path():
    from diffmusic_amd import ops
    h = ops.load()
    for case in (STFT_CASES[1], STFT_CASES[2]):
        name, L, full, hop, hann, power2, to_db, lo, hi, masked, shared = case
        fe, wav, mask, ref, kw, sigma, B = _kernel_problem(case)
        st = fe._get_state(B, L, wav.device)
        args = (fe._h.value, wav, mask, ref, st, L, full, power2, to_db, lo, hi, 0.5, kw.get("noise"), kw.get("noise_mag"), sigma)
        a, b = h.mel_guidance(*args), ops.ctypes_hip.mel_guidance(*args)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name
        plain = h.mel_guidance(*args[:12])
        assert not torch.equal(plain[0], a[0])
        quiet = h.mel_guidance(*args[:12], None, None, 0.0)                       # no additive input: the bits of the defaults
        assert torch.equal(quiet[0], plain[0]) and torch.equal(quiet[1], plain[1])
    g = torch.Generator().manual_seed(2)
    for n, shift in ((4096, 0), (4099, 0), (3, 0), (1001, 1)):                    # float4 body + tail, tiny, and a 4-byte-aligned pointer
        buf_y, buf_z = torch.randn(n + shift, generator=g).cuda(), torch.randn(n + shift, generator=g).cuda()
        yv, zv = buf_y[shift:], buf_z[shift:]
        assert yv.is_contiguous() and yv.data_ptr() % 16 == (4 * shift) % 16
        a, b = h.noise_add(yv, zv, 0.37), ops.ctypes_hip.noise_add(yv, zv, 0.37)
        assert torch.equal(a, b) and a.shape == yv.shape
        assert _rel(a, yv.double() + 0.37 * zv.double()) < 1e-6
    with pytest.raises(RuntimeError, match="size / device mismatch"):
        h.noise_add(torch.zeros(8).cuda(), torch.zeros(9).cuda(), 1.0)


# ---- 8: sigma = 0 changes nothing -----------------------------------------------------------------------------------------------------
def test_sigma_zero_step_equals_a_step_without_noiser(nets):
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    voc, vae, _, _ = nets
    g = torch.Generator().manual_seed(78)
    clean = (0.3 * torch.sin(torch.arange(LEN) * 0.05)[None] + 0.05 * torch.randn(2, LEN, generator=g)).cuda()
    x, e = torch.randn(2, 8, H, W, generator=g).cuda(), torch.randn(2, 8, H, W, generator=g).cuda()
    outs = []
    for space in ("mel_spectrogram", "wav_form"):
        for noiser in (None, P.GaussianNoise(0.0), P.GaussianNoise(0.0, stream="clip"), P.PoissonNoise(1.0)):
            op = P.MusicInpaintingOperator(1, LEN, "box", 0.25, 0.5, 0.3, 0.1, 0.2, noiser=noiser)
            sched = get_scheduler("dps")(operator=op, **SCHED)
            sched.set_timesteps(200)
            y = (clean * op.mask.cuda()).contiguous()
            before = torch.get_rng_state()
            out = sched.step(e, 501, x, eta=0.0, ip_guidance_rate=5e-4, measurement=y, vae=vae, vocoder=voc, original_waveform_length=LEN,
                             supervised_space=space, generator=[torch.Generator().manual_seed(k) for k in range(2)])
            assert torch.equal(torch.get_rng_state(), before)                     # no draw from the global stream either
            outs.append((out.prev_sample.clone(), out.loss.clone()))
        for prev, loss in outs[1:]:
            assert torch.equal(prev, outs[0][0]) and torch.equal(loss, outs[0][1]), space
        outs = []
