"""-m gpu: track mode (diffmusic_amd/inverse_problem/track.py, csrc/track.hip) -- one recording as W overlapping windows under one loss.

Kernel level: S and S^T against a float64 restatement, the adjoint identity, both bindings, and the inner fused guidance at the
length of an 8-window track.  Step level: teacher-forced steps against `oracle.schedulers` with `per_clip_norm=False` around a
wrapper whose `forward` stitches in torch and calls the oracle operator (`OracleTrack` below); before that, on the oracle alone,
the track's loss differs from the whole-batch norm of the windows scored on their own by more than twice the loss bound, so a product
that skipped the stitch cannot pass.  Call level: `pipe(...)` in track mode equals a hand-written loop bit for bit, cold, warm-started
and with a NaN restart; W = 1 equals the ordinary call; one production-size run against the oracle loop."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_track_host import weights64                                          # noqa: E402
from tests.test_gpu_step import HIFI, VAE, SCHED, H, W as LAT_W, LEN               # noqa: E402

_NEG, _POS = -3.0e38, 3.0e38
T3, R3 = 16000, 1600                      # W = 3 windows of LEN = 6400 at 0, 4800, 9600: overlaps of exactly R
EPS32 = 2.0 ** -23


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-300))


def _dot(a, b):
    return float((a.double().cpu().reshape(-1) * b.double().cpu().reshape(-1)).sum())


class OracleTrack:
    """The oracle-side TrackOperator: `forward` stitches the (W, L) windows in torch (differentiable, the float64 weights of
    tests/test_track_host.py::weights64 in the waveform's dtype) and calls the oracle operator on the (1, T) track."""

    def __init__(self, inner, layout):
        self.inner, self.layout = inner, layout
        self.wt = torch.from_numpy(weights64(layout))

    def stitch(self, wav):
        lay, L = self.layout, self.layout.window_len
        track = torch.zeros(lay.track_len, dtype=wav.dtype)
        for w, s in enumerate(lay.starts):
            track = track + torch.nn.functional.pad(self.wt[w, s:s + L].to(wav.dtype) * wav[w, :L], (s, lay.track_len - s - L))
        return track[None]

    def forward(self, wav, **k):
        return self.inner.forward(self.stitch(wav), **k)

    def transform(self, x):
        return self.inner.transform(x)

    def inverse_transform(self, mel, vocoder):
        return self.inner.inverse_transform(mel, vocoder)


def _layout(T, L, R):
    from diffmusic_amd.inverse_problem import TrackLayout
    return TrackLayout(T, L, R)


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------
KERNEL_CASES = [(3, 6400, 1600, 16000, 32), (3, 6400, 1600, 11300, 32), (3, 6400, 1600, 11300, 37), (8, 163840, 20480, 1167360, 32)]


def _windows(W, full, seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.arange(full, dtype=torch.float32)
    x = torch.stack([0.4 * torch.sin(n * (0.01 + 0.003 * w) + w) for w in range(W)]) + 0.1 * torch.randn(W, full, generator=g)
    x[0, 5] = -0.0                                                                   # a signed zero must survive the copy
    return x.cuda()


@pytest.mark.parametrize("W,L,R,T,pad", KERNEL_CASES)
def test_stitch_matches_float64_and_copies_single_cover_samples(W, L, R, T, pad):
    from diffmusic_amd import ops
    lay = _layout(T, L, R)
    assert lay.num_windows == W
    full = L + pad
    wav = _windows(W, full, 1)                                                       # row stride full > L
    track = ops.hip.track_stitch_fwd(wav, lay.starts, L, R, T)
    assert track.shape == (1, T) and track.dtype == torch.float32
    wt = torch.from_numpy(weights64(lay))
    want = torch.zeros(T, dtype=torch.float64)
    cover = torch.zeros(T, dtype=torch.int64)
    for w, s in enumerate(lay.starts):
        want[s:s + L] += wt[w, s:s + L] * wav[w, :L].double().cpu()
        cover[s:s + L] += 1
    if T == 11300:
        assert int(cover.max()) == 3                                                 # the three-cover layout
    r = _rel(track[0], want)
    print(f"\n  S (W={W}, L={L}, R={R}, T={T}, stride {full}): rel-L2 vs float64 {r:.2e}")
    assert r < 1e-6
    got = track[0].cpu()
    single = cover == 1
    owner = torch.zeros(T, dtype=torch.int64)
    for w, s in enumerate(lay.starts):
        owner[s:s + L][single[s:s + L]] = w
    n = torch.nonzero(single).reshape(-1)
    src = wav.cpu()[owner[n], n - torch.tensor(lay.starts)[owner[n]]]
    assert torch.equal(got[n].view(torch.int32), src.view(torch.int32))              # bit for bit, -0.0 included
    ones = ops.hip.track_stitch_fwd(torch.ones(W, full, device="cuda"), lay.starts, L, R, T)[0].cpu()
    assert bool((ones[single] == 1.0).all())
    worst = float((ones.double() - 1.0).abs().max())
    print(f"  S(ones): worst |x - 1| = {worst / EPS32:.2f} ulp")
    assert worst <= 2 * EPS32
    sliced = ops.hip.track_stitch_fwd(wav[:, 1:], lay.starts, L, R, T) if pad > 1 else None     # rows 4 bytes off 16-byte alignment
    if sliced is not None:
        want1 = torch.zeros(T, dtype=torch.float64)
        for w, s in enumerate(lay.starts):
            want1[s:s + L] += wt[w, s:s + L] * wav[w, 1:L + 1].double().cpu()
        assert _rel(sliced[0], want1) < 1e-6


@pytest.mark.parametrize("W,L,R,T,pad", KERNEL_CASES)
def test_stitch_transpose_is_the_adjoint(W, L, R, T, pad):
    from diffmusic_amd import ops
    lay = _layout(T, L, R)
    full = L + pad
    g = torch.Generator().manual_seed(7)
    x = torch.randn(W, full, generator=g).cuda()
    y = torch.randn(1, T, generator=g).cuda()
    sx = ops.hip.track_stitch_fwd(x, lay.starts, L, R, T)
    sty = ops.hip.track_stitch_bwd(y, lay.starts, L, R, full)
    assert sty.shape == (W, full)
    assert float(sty[:, L:].abs().max()) == 0.0                                      # the tail past L is exactly zero
    lhs, rhs = _dot(sx, y), _dot(x[:, :L], sty[:, :L])
    print(f"\n  <S x, y> = {lhs:.6f}, <x, S^T y> = {rhs:.6f}")
    assert abs(lhs - rhs) <= 2e-4 * max(abs(lhs), abs(rhs), math.sqrt(x[:, :L].numel())), (lhs, rhs)
    wt = torch.from_numpy(weights64(lay))
    want = torch.stack([wt[w, s:s + L] * y[0, s:s + L].double().cpu() for w, s in enumerate(lay.starts)])
    assert _rel(sty[:, :L], want) < 1e-6
    # a tail of NaNs in a reused buffer would poison the vocoder backward: the kernel writes the zeros itself
    assert bool(torch.isfinite(sty).all())


def test_both_bindings_are_bit_identical_and_refuse_bad_layouts():
    from diffmusic_amd import ops
    h = ops.load()
    for W, L, R, T, pad in KERNEL_CASES[:3]:
        lay = _layout(T, L, R)
        wav = _windows(W, L + pad, 3)
        a, b = h.track_stitch_fwd(wav, lay.starts, L, R, T), ops.ctypes_hip.track_stitch_fwd(wav, lay.starts, L, R, T)
        assert torch.equal(a, b) and a.shape == b.shape == (1, T)
        y = torch.randn(1, T, generator=torch.Generator().manual_seed(4)).cuda()
        a, b = h.track_stitch_bwd(y, lay.starts, L, R, L + pad), ops.ctypes_hip.track_stitch_bwd(y, lay.starts, L, R, L + pad)
        assert torch.equal(a, b) and a.shape == (W, L + pad)
    wav = _windows(3, 6432, 3)
    for fn in (h.track_stitch_fwd, ops.ctypes_hip.track_stitch_fwd):
        with pytest.raises(RuntimeError, match="first window starts at 0"):
            fn(wav, [1, 4800, 9600], 6400, 1600, 16000)
        with pytest.raises(RuntimeError, match="increase by less than L"):
            fn(wav, [0, 6400, 9600], 6400, 1600, 16000)                              # a gap: a sample nobody covers
        with pytest.raises(RuntimeError, match="R <= L / 2"):
            fn(wav, [0, 4800, 9600], 6400, 3201, 16000)
    for fn in (h.track_stitch_bwd, ops.ctypes_hip.track_stitch_bwd):
        with pytest.raises(RuntimeError, match="full >= L"):
            fn(torch.zeros(1, 16000).cuda(), [0, 4800, 9600], 6400, 1600, 6399)


@pytest.mark.parametrize("masked", [True, False], ids=["inpainting_mask", "identity"])
def test_inner_fused_guidance_at_track_length(masked):
    """The fused STFT -> mel guidance pair at B = 1, T = 1 167 360 (the 8-window layout) against the float64 `_truth` of
    tests/test_gpu_noise.py, with that file's bounds."""
    import bench
    from diffmusic_amd.inverse_problem import dsp
    from diffmusic_amd.inverse_problem.operator import SpectralFrontend
    from tests.test_gpu_noise import _truth
    T = _layout(1167360, 163840, 20480).track_len
    fe = SpectralFrontend(16000, 1024, 160, 64, "hann")
    assert fe.fused(T)
    fb = torch.from_numpy(dsp.melscale_fbanks(513, 0.0, 8000.0, 64, 16000)).cuda()
    wav = (bench.synth_clip(3, T) + 0.05 * torch.randn(T, generator=torch.Generator().manual_seed(9)))[None].cuda().contiguous()
    target = bench.synth_clip(4, T)[None].cuda().contiguous()
    mask = None
    lo, hi = (-80.0, 80.0)
    if masked:
        lo, hi = _NEG, _POS
        mask = torch.ones(T)
        for k in range(1, 8):                                                        # a gap across every cut of the 8-window layout
            mask[k * 143360 + 2000: k * 143360 + 18000] = 0.0
        mask[:300] = 0.0
        mask = mask.cuda()
    ref = fe.transform_fwd(target, T, True, True, lo, hi).clone()
    _, loss_t, g_t = _truth(wav, mask, fb, ref, T, 160, True, True, True, max(lo, -1e300), min(hi, 1e300))
    loss, dwav = fe.guidance(wav, T, ref, mask, True, True, lo, hi)
    assert loss.shape == (1,) and dwav.shape == (1, T)
    rl = float(((loss.double() - loss_t).abs() / loss_t).max())
    rg, r0, r1 = _rel(dwav, g_t), _rel(dwav[:, :600], g_t[:, :600]), _rel(dwav[:, T - 600:], g_t[:, T - 600:])
    print(f"\n  fused guidance at T={T} ({'mask' if masked else 'identity'}): loss {rl:.2e} grad {rg:.2e} first600 {r0:.2e} last600 {r1:.2e}")
    assert rl < 2e-5, (loss, loss_t)
    assert rg < 2e-4
    assert r0 < 5e-4 and r1 < 5e-4
    if mask is not None:
        assert float(dwav[0][mask == 0].abs().max()) == 0.0


# ---- step level -------------------------------------------------------------------------------------------------------------------------
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
    def __init__(self, sigma, z):
        self.sigma, self.z = sigma, z

    def __call__(self, data):
        return data + self.sigma * self.z


GAP = (0.28, 0.42)                        # of a 16 000-sample track: samples 4480 ... 6720, across the first overlap [4800, 6400)


def _track_ops(task, T, sigma=0.0):
    """(product operator, oracle operator), both built for the TRACK's length."""
    from diffmusic_amd import inverse_problem as P
    from oracle import operators as O
    n, rn = P.get_noiser("gaussian", sigma), O.get_noiser("gaussian", 0.0)
    if task == "music_inpainting":
        args = (1, T, "box", GAP[0], GAP[1], 0.3, 0.1, 0.2)
        return P.MusicInpaintingOperator(*args, noiser=n), O.MusicInpaintingOperator(*args, noiser=rn)
    if task == "phase_retrieval":
        return P.PhaseRetrievalOperator(noiser=n), O.PhaseRetrievalOperator(noiser=rn)
    if task == "super_resolution4":
        return P.SuperResolutionOperator(16000, 4, noiser=n), O.SuperResolutionOperator(16000, 4, noiser=rn)
    assert task == "music_dereverberation"
    return P.MusicDereverberationOperator(500, 0.99, noiser=n), O.MusicDereverberationOperator(500, 0.99, noiser=rn)


def _clean_track(T, seed=77):
    g = torch.Generator().manual_seed(seed)
    return (0.3 * torch.sin(torch.arange(T) * 0.05) + 0.05 * torch.randn(T, generator=g))[None], g


def oracle_gap(nets, task, lay, rop, y_ref, x0, opk):
    """On the oracle alone: (loss of the stitched track, whole-batch norm of the windows scored separately against their slices of the
    measurement), mel space.  Window w is scored with what a hand-cut batch would use: its slice of the mask / the same impulse response."""
    _, _, rvoc, rvae = nets
    L = lay.window_len
    with torch.no_grad():
        wav = rop.inverse_transform(rvae.decode(x0 / rvae.config.scaling_factor).sample, rvoc)[:, :L]
        track = OracleTrack(rop, lay).stitch(wav)
        whole = torch.linalg.norm(rop.transform(y_ref) - rop.transform(rop.forward(track, **opk)))
        parts = []
        for w, s in enumerate(lay.starts):
            if task == "music_inpainting":
                a_w, y_w = wav[w:w + 1] * rop.mask[:, s:s + L], y_ref[:, s:s + L]
            else:
                a_w = rop.forward(wav[w:w + 1], **opk)
                y_w = y_ref[:, s:s + a_w.shape[1]]
            parts.append(torch.linalg.norm(rop.transform(y_w) - rop.transform(a_w)))
        return float(whole), float(torch.linalg.norm(torch.stack(parts)))


STEP_CASES = [("dps", "music_inpainting", 0.0, 5e-4, "mel_spectrogram", 501, 0.0),
              ("dps", "music_dereverberation", 0.0, 5e-4, "mel_spectrogram", 501, 0.0),
              ("mpgd", "super_resolution4", 0.0, 5e-3, "mel_spectrogram", 501, 0.0),
              ("dsg", "phase_retrieval", 1.0, 0.08, "mel_spectrogram", 501, 0.0),
              ("dps", "music_inpainting", 0.0, 5e-4, "wav_form", 996, 0.0),
              ("dps", "music_inpainting", 0.0, 5e-4, "mel_spectrogram", 501, 0.05)]


@pytest.mark.parametrize("name,task,eta,rate,space,t,sigma", STEP_CASES, ids=[f"{c[0]}-{c[1]}-{c[4]}-sigma{c[6]}" for c in STEP_CASES])
def test_teacher_forced_track_step(nets, name, task, eta, rate, space, t, sigma):
    """`_teacher_forced` of tests/test_gpu_step.py on a 3-window track: same x, eps and noise on both sides, its bounds
    (loss < 1e-2, prev_sample rel-L2 < 1e-2, gradient cosine > 0.98)."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    from oracle import schedulers as OS
    voc, vae, rvoc, rvae = nets
    lay = _layout(T3, LEN, R3)
    Wn = lay.num_windows
    assert Wn == 3 and lay.starts == [0, 4800, 9600]
    op, rop = _track_ops(task, T3, sigma)
    clean, g = _clean_track(T3)
    opk = dict(ir=rop.generate_impulse_response(500, 0.99)) if task == "music_dereverberation" else {}
    x = torch.randn(Wn, 8, H, LAT_W, generator=g)
    e = torch.randn(Wn, 8, H, LAT_W, generator=g)
    z = torch.randn(Wn, 8, H, LAT_W, generator=g)
    y_ref = rop.forward(clean, **opk)
    z_step = None
    if sigma > 0:
        z_meas, z_step = torch.randn(y_ref.shape, generator=g), torch.randn(y_ref.shape, generator=g)
        y_ref = y_ref + sigma * z_meas                                              # the measurement's own draw, made once
        y = y_ref.cuda()
    else:
        y = op.forward(clean.cuda(), **opk)
        assert _rel(y, y_ref) < 1e-4, "operator.forward at track length"
    rs = OS.get_scheduler(name)(operator=OracleTrack(rop, lay), per_clip_norm=False, **SCHED)
    rs.set_timesteps(200)
    if space == "mel_spectrogram" and sigma == 0 and task in ("music_inpainting", "music_dereverberation"):
        a_t = float(rs.alphas_cumprod[t])
        whole, separate = oracle_gap(nets, task, lay, rop, y_ref, (x - (1 - a_t) ** 0.5 * e) / a_t ** 0.5, opk)
        gap = abs(whole - separate) / whole
        print(f"\n  {task}: oracle loss of the track {whole:.4f}, of the windows scored separately {separate:.4f}: {gap:.3f} apart")
        assert gap > 2e-2, (whole, separate)
    if sigma > 0:
        rop.noiser = _FixedNoiser(sigma, z_step)
    kw = dict(eta=eta, ip_guidance_rate=rate, original_waveform_length=LEN, supervised_space=space)
    rnoise = dict(sample_noise=z) if name in ("dsg", "diffmusic") else dict(variance_noise=z if eta > 0 else None)
    ro = rs.step(e, t, x, measurement=y_ref, vae=rvae, vocoder=rvoc, op_kwargs=opk, **kw, **rnoise)
    assert ro.loss.numel() == 1
    sched = get_scheduler(name)(operator=P.TrackOperator(op, lay), per_clip_norm=False, **SCHED)
    sched.set_timesteps(200)
    sched.debug_keep_grad = True
    noise_kw = dict(sample_noise=z.cuda()) if name in ("dsg", "diffmusic") else dict(variance_noise=z.cuda() if eta > 0 else None)
    popk = dict(opk, noise=z_step.cuda()) if sigma > 0 else opk
    out = sched.step(e.cuda(), t, x.cuda(), measurement=y, vae=vae, vocoder=voc, op_kwargs=popk, **kw, **noise_kw)
    torch.cuda.synchronize()
    assert out.loss.numel() == 1 and out.prev_sample.shape == x.shape
    rp = _rel(out.prev_sample, ro.prev_sample)
    rl = _rel(out.loss.reshape(-1), ro.loss.reshape(-1))
    rg = _rel(sched.last_grad, ro.sample)
    cos = torch.nn.functional.cosine_similarity(sched.last_grad.cpu().flatten(), ro.sample.flatten(), dim=0).item()
    msg = f"track {name}/{task}/{space}/sigma={sigma}: prev {rp:.2e} loss {rl:.2e} grad {rg:.2e} cos {cos:.4f}"
    print("  " + msg)
    assert _rel(out.pred_original_sample, ro.pred_original_sample) < 1e-4 or name == "mpgd"
    assert rl < 1e-2, msg
    assert cos > 0.98, msg
    assert rp < 1e-2, msg
    assert all(float(sched.last_grad[w].abs().max()) > 0 for w in range(Wn)), "the gradient reaches every window"


def test_per_clip_norm_scheduler_is_refused_at_step(nets):
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    voc, vae, _, _ = nets
    lay = _layout(T3, LEN, R3)
    op, _ = _track_ops("music_inpainting", T3)
    sched = get_scheduler("dps")(operator=P.TrackOperator(op, lay), **SCHED)
    sched.set_timesteps(200)
    x = torch.randn(3, 8, H, LAT_W).cuda()
    with pytest.raises(ValueError, match="per_clip_norm=False"):
        sched.step(x, 501, x, measurement=torch.zeros(1, T3).cuda(), vae=vae, vocoder=voc, original_waveform_length=LEN)


def test_one_window_track_equals_the_plain_operator_bit_for_bit(nets):
    """T == L: the weight is u / u == 1.0f, so stitch and its transpose are copies and everything else is the same launches."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    voc, vae, _, _ = nets
    lay = _layout(LEN, LEN, R3)
    assert lay.num_windows == 1
    g = torch.Generator().manual_seed(5)
    clean = 0.3 * torch.sin(torch.arange(LEN) * 0.05)[None] + 0.05 * torch.randn(1, LEN, generator=g)
    wav = (0.2 * torch.randn(1, LEN + 32, generator=g)).cuda()
    x, e = torch.randn(1, 8, H, LAT_W, generator=g).cuda(), torch.randn(1, 8, H, LAT_W, generator=g).cuda()
    for space in ("mel_spectrogram", "wav_form"):
        args = (1, LEN, "box", 0.25, 0.5, 0.3, 0.1, 0.2)
        plain = P.MusicInpaintingOperator(*args, noiser=P.get_noiser("gaussian", 0.0))
        inner = P.MusicInpaintingOperator(*args, noiser=P.get_noiser("gaussian", 0.0))
        track = P.TrackOperator(inner, lay)
        y = plain.forward(clean.cuda())
        l0, d0 = plain.guidance(wav, LEN, y, space)
        l1, d1 = track.guidance(wav, LEN, y, space)
        assert l1.shape == (1,) and d1.shape == d0.shape == (1, LEN + 32)
        assert torch.equal(l0, l1) and torch.equal(d0, d1), space
        outs = []
        for op in (plain, track):
            s = get_scheduler("dps")(operator=op, per_clip_norm=False, **SCHED)
            s.set_timesteps(200)
            outs.append(s.step(e, 501, x, measurement=y, vae=vae, vocoder=voc, original_waveform_length=LEN, supervised_space=space))
        assert torch.equal(outs[0].prev_sample, outs[1].prev_sample) and torch.equal(outs[0].loss, outs[1].loss), space


# ---- call level -------------------------------------------------------------------------------------------------------------------------
N_CALL, SECONDS = 10, 0.4


def _track_pipe(kind="musicldm", T=T3, plain=False):
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.pipelines import get_pipeline
    from diffmusic_amd.schedulers import get_scheduler
    from tests.test_gpu_warm_start import HIFI as HIFI_SR, UNET
    unet = UNET if kind == "musicldm" else dict(UNET, class_embed_dim=0, attn_cross_dims=[0, 48, 64])
    pipe = get_pipeline(kind).from_pretrained("synthetic", seed=0, unet_config=unet, vae_config=VAE, vocoder_config=HIFI_SR).to("cuda")
    lay = _layout(T, LEN, R3)
    gap = GAP if T == T3 else (0.25, 0.5)
    inner = P.MusicInpaintingOperator(1, T, "box", gap[0], gap[1], 0.3, 0.1, 0.2, noiser=P.get_noiser("gaussian", 0.0))
    op = inner if plain else P.TrackOperator(inner, lay)
    pipe.scheduler = get_scheduler("dps")(operator=op, per_clip_norm=False, **SCHED)
    pipe.assume_uncond_equals_cond = True
    return pipe, op, lay


def _call_inputs(kind, Wn, T, seed=21):
    clean, g = _clean_track(T, seed)
    if kind == "musicldm":
        cond = dict(prompt_embeds=torch.nn.functional.normalize(torch.randn(Wn, 512, generator=g), dim=-1))
    else:
        cond = dict(prompt_embeds=torch.randn(Wn, 10, 64, generator=g), attention_mask=torch.ones(Wn, 10),
                    generated_prompt_embeds=torch.randn(Wn, 8, 48, generator=g))
    return clean, cond


def _gens(Wn):
    return [torch.Generator().manual_seed(300 + k) for k in range(Wn)]


def _hand_loop(pipe, top, lay, cond, y, gscale, timesteps=None, x=None):
    """`_unet_eps` + `scheduler.step` + decode + `stitch`, written out; returns (track (1, T), latents, losses)."""
    dev = torch.device("cuda")
    s = pipe.scheduler
    Wn = lay.num_windows
    gens = _gens(Wn)
    if x is None:
        s.set_timesteps(N_CALL, device="cuda")
        timesteps = list(s._timesteps_host)
        x = pipe.prepare_latents(Wn, 8, 40, torch.float32, dev, gens, None)
    else:
        x, gens = x
    if "generated_prompt_embeds" in cond:
        c = pipe._prepare_cond(cond["prompt_embeds"], None, 1, True, dev, generated_prompt_embeds=cond["generated_prompt_embeds"],
                               attention_mask=cond["attention_mask"])
    else:
        c = pipe._prepare_cond(cond["prompt_embeds"], None, 1, True, dev)
    losses = []
    for t in timesteps:
        eps = pipe._unet_eps(x, t, c, gscale, True)
        o = s.step(eps, t, x, eta=0.0, generator=gens, measurement=y, vae=pipe.vae, vocoder=pipe.vocoder, original_waveform_length=LEN,
                   ip_guidance_rate=5e-4, supervised_space="mel_spectrogram")
        x = o.prev_sample
        losses.append(o.loss)
    wav = pipe.vocoder(pipe.vae.decode(x / pipe.vae.config.scaling_factor).sample.squeeze(1)).float()
    return top.stitch(wav), x, losses


@pytest.mark.parametrize("kind", ["musicldm", "audioldm2"])
def test_track_call_equals_the_hand_written_loop(kind):
    pipe, top, lay = _track_pipe(kind)
    Wn = lay.num_windows
    clean, cond = _call_inputs(kind, Wn, T3)
    y = top.forward(clean.cuda())
    gscale = pipe.default_guidance_scale
    call = dict(audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0, **cond)
    out = pipe(generator=_gens(Wn), output_type="pt", **call).audios
    assert out.shape == (1, T3) and pipe.nan_restarts == 0
    assert len(pipe.last_losses) == N_CALL and all(l.numel() == 1 for l in pipe.last_losses)      # one loss for the whole track
    lat = pipe(generator=_gens(Wn), output_type="latent", **call).audios
    assert lat.shape == (Wn, 8, 10, 16)
    track, x, losses = _hand_loop(pipe, top, lay, cond, y, gscale)
    assert torch.equal(lat, x)
    assert torch.equal(out, track.cpu())
    assert all(torch.equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(pipe.last_losses, losses))
    assert out.abs().max() > 0 and bool(torch.isfinite(out).all())


def test_warm_started_track_call_equals_its_hand_loop():
    """`init_audio=layout.cut(y)`, `strength=0.5`: 5 of 10 steps, from the encoded windows of the measurement."""
    from diffmusic_amd.torch_utils import randn_tensor
    pipe, top, lay = _track_pipe()
    Wn = lay.num_windows
    clean, cond = _call_inputs("musicldm", Wn, T3)
    y = top.forward(clean.cuda())
    init = lay.cut(y)
    assert init.shape == (Wn, LEN)
    out = pipe(audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0, generator=_gens(Wn),
               output_type="pt", init_audio=init, strength=0.5, **cond).audios
    assert len(pipe.last_losses) == 5 and out.shape == (1, T3)
    s = pipe.scheduler
    s.set_timesteps(N_CALL, device="cuda")
    ts = s.timesteps_for_strength(0.5)
    assert ts == list(s._timesteps_host)[5:]
    gens = _gens(Wn)
    dev = torch.device("cuda")
    z0 = pipe._encode_init(init, True, "sample", gens, LEN, 40, dev)
    noise = randn_tensor(z0.shape, generator=gens, device=dev, dtype=torch.float32)
    x = s.add_noise(z0, noise, ts[0])
    track, _, _ = _hand_loop(pipe, top, lay, cond, y, 2.0, timesteps=ts, x=(x, gens))
    assert torch.equal(out, track.cpu())


def test_nan_restarts_all_windows():
    pipe, top, lay = _track_pipe()
    Wn = lay.num_windows
    clean, cond = _call_inputs("musicldm", Wn, T3)
    y = top.forward(clean.cuda())
    real_step = pipe.scheduler.step
    state = dict(calls=0, first=[])

    def step(model_output, timestep, sample, **kw):
        out = real_step(model_output, timestep, sample, **kw)
        if timestep == pipe.scheduler._timesteps_host[0]:
            state["first"].append(sample.clone())
        if state["calls"] == 2:
            out.loss = out.loss * float("nan")
        state["calls"] += 1
        return out
    pipe.scheduler.step = step
    out = pipe(audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0, generator=_gens(Wn),
               output_type="pt", **cond).audios
    assert pipe.nan_restarts == 1 and state["calls"] == 3 + N_CALL
    a, b = state["first"]
    assert bool((a != b).flatten(1).any(dim=1).all())                                # every window's latent was redrawn
    assert out.shape == (1, T3) and bool(torch.isfinite(out).all())


def test_one_window_call_equals_the_ordinary_call():
    tp, top, lay = _track_pipe(T=LEN)
    pp, pop, _ = _track_pipe(T=LEN, plain=True)
    assert lay.num_windows == 1
    clean, cond = _call_inputs("musicldm", 1, LEN)
    outs = []
    for pipe, op in ((pp, pop), (tp, top)):
        y = op.forward(clean.cuda())
        outs.append(pipe(audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0,
                         generator=_gens(1), output_type="pt", **cond).audios)
        outs.append(torch.stack([l.reshape(()) for l in pipe.last_losses]))
    assert outs[0].shape == outs[2].shape == (1, LEN)
    assert torch.equal(outs[1], outs[3]) and torch.equal(outs[0], outs[2])


def test_fullsize_two_window_track_against_the_oracle_loop():
    """Built like tests/test_gpu_noise.py::test_fullsize_noisy_short_trajectory_snr: the networks of `bench.build_problem`, N = 10, DPS
    inpainting, W = 2 windows of the benchmark length with R = 1.28 s on an 18 s track (starts 0 and 8 s), a box gap from 7.75 s to
    8.75 s across the cut, the operator built for the track's length.  Against the oracle loop with the track wrapper: waveform SNR of
    the stitched track >= 30 dB and every step's loss within 1e-2."""
    import bench
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    from oracle import operators as OO, schedulers as OS
    from tests.test_gpu_batch_parity import _snr_db
    from tests.test_gpu_fullsize_parity import _oracle_nets
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    dev = torch.device("cuda")
    wl, N = "dps_inpainting", 10
    pname, sname, eta, rate, task, _, _ = bench.WORKLOADS[wl]
    pipe, _, _, lat, cond, L = bench.build_problem(2, 0, dev, wl)
    T, R = 18 * bench.SR, int(1.28 * bench.SR)
    lay = _layout(T, L, R)
    assert lay.num_windows == 2 and lay.starts == [0, 128000]
    args = (18, bench.SR, "box", 7.75, 8.75, 0.3, 0.1, 1.0)
    inner = P.MusicInpaintingOperator(*args, noiser=P.get_noiser("gaussian", 0.0))
    assert inner.mask.shape == (1, T)
    top = P.TrackOperator(inner, lay)
    pipe.scheduler = get_scheduler(sname)(operator=top, per_clip_norm=False, **bench.SCHED_CFG)
    clean = bench.synth_clip(0, T)[None]
    meas = top.forward(clean.to(dev))
    pe = cond["class_labels"][:2]
    out = pipe(prompt_embeds=pe, negative_prompt_embeds=pe, audio_length_in_s=bench.SECONDS, num_inference_steps=N,
               guidance_scale=bench.GUIDANCE_SCALE, latents=lat.clone(), measurement=meas, ip_guidance_rate=rate, eta=eta,
               show_progress=False, output_type="pt")
    assert out.audios.shape == (1, T) and pipe.nan_restarts == 0
    hip_losses = [float(l.reshape(-1)[0]) for l in pipe.last_losses]
    ru, rv, rh = _oracle_nets(pipe, wl)
    rop = OO.MusicInpaintingOperator(*args, noiser=OO.get_noiser("gaussian", 0.0))
    otrack = OracleTrack(rop, lay)
    yr = rop.forward(clean)
    rs = OS.get_scheduler(sname)(operator=otrack, per_clip_norm=False, **bench.SCHED_CFG)
    rs.set_timesteps(N)
    x, pec = lat.cpu().float(), pe.cpu()
    losses = []
    for t in [int(v) for v in rs.timesteps]:
        with torch.no_grad():
            e2 = ru(torch.cat([x, x]), t, class_labels=torch.cat([pec, pec]))[0]
        e = e2[:2] + bench.GUIDANCE_SCALE * (e2[2:] - e2[:2])
        so = rs.step(e, t, x, eta=eta, measurement=yr, vae=rv, vocoder=rh, original_waveform_length=L, ip_guidance_rate=rate,
                     supervised_space="mel_spectrogram")
        x = so.prev_sample.detach()
        losses.append(float(so.loss.reshape(-1)[0]))
    with torch.no_grad():
        track = otrack.stitch(rh(rv.decode(x / rv.config.scaling_factor).sample.squeeze(1))[:, :L])
    snr = _snr_db(track, out.audios)
    lrel = max(abs(a - b) / abs(b) for a, b in zip(hip_losses, losses))
    print(f"\n  2-window track, N={N}, full size: waveform SNR of the stitched track vs the oracle loop {snr:.1f} dB; worst per-step loss "
          f"rel err {lrel:.2e}")
    assert snr >= 30.0
    assert lrel < 1e-2
