"""-m gpu: the HIP VAE encoder (csrc/vae_enc.hip) against a test-local fp32 torch restatement of diffusers' AutoencoderKL.encode
assembled from the oracle's blocks, the asymmetric-pad stride-2 convolution alone, batch invariance, the `latent_init` output stage,
both bindings, and the model-domain mel front end against a float64 restatement of its own definition.

Measured on MI355X (relative L2 of the moments against the fp32 restatement; bound 1e-2, the decoder measures 1.0e-3): see
profiles/vae_encoder_parity.json."""
import ctypes as C
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SMALL = dict(latent_channels=8, out_channels=1, block_out_channels=[32, 64, 64], layers_per_block=2, norm_num_groups=32,
             scaling_factor=0.9227914214134216, eps=1e-6)


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


class RefEncoder(nn.Module):
    """diffusers 0.31 `AutoencoderKL.encode` up to the moments: Encoder (DownEncoderBlock2D x n, mid block, norm / SiLU / conv_out) and
    quant_conv, with the checkpoint's tensor names."""

    def __init__(self, latent_channels, out_channels, block_out_channels, layers_per_block, norm_num_groups, eps, **_):
        super().__init__()
        from oracle.models import ResnetBlock2D, _MidBlock
        boc, g = list(block_out_channels), norm_num_groups
        enc = nn.Module()
        enc.conv_in = nn.Conv2d(out_channels, boc[0], 3, padding=1)
        enc.down_blocks = nn.ModuleList()
        prev = boc[0]
        for i, c in enumerate(boc):
            blk = nn.Module()
            blk.resnets = nn.ModuleList([ResnetBlock2D(prev if j == 0 else c, c, None, g, eps) for j in range(layers_per_block)])
            if i != len(boc) - 1:
                ds = nn.Module()
                ds.conv = nn.Conv2d(c, c, 3, stride=2, padding=0)
                blk.downsamplers = nn.ModuleList([ds])
            enc.down_blocks.append(blk)
            prev = c
        enc.mid_block = _MidBlock(boc[-1], g, eps)
        enc.conv_norm_out = nn.GroupNorm(g, boc[-1], eps=eps)
        enc.conv_out = nn.Conv2d(boc[-1], 2 * latent_channels, 3, padding=1)
        self.encoder = enc
        self.quant_conv = nn.Conv2d(2 * latent_channels, 2 * latent_channels, 1)

    def forward(self, mel):                                   # (B, T, F) -> moments (B, h * w, 2L), channels-last like the engine's
        e = self.encoder
        x = e.conv_in(mel[:, None])
        for blk in e.down_blocks:
            for r in blk.resnets:
                x = r(x)
            if hasattr(blk, "downsamplers"):
                x = blk.downsamplers[0].conv(F.pad(x, (0, 1, 0, 1)))          # Downsample2D(padding=0)
        x = e.conv_out(F.silu(e.conv_norm_out(e.mid_block(x))))
        m = self.quant_conv(x)
        return m.permute(0, 2, 3, 1).reshape(m.shape[0], -1, m.shape[1])


def _pair(cfg, seed=4):
    from diffmusic_amd.engine import VaeEncoderEngine
    eng = VaeEncoderEngine(cfg)
    sd = eng.synth_state_dict(seed=seed)
    eng.load_state_dict(sd, strict=True)
    ref = RefEncoder(**eng.cfg).eval()
    ref.load_state_dict(sd, strict=True)
    return eng, ref                                   # the restatement runs on the CPU in fp32


def _mel(B, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (2.0 * torch.randn(B, T, 64, generator=g) - 4.0).cuda()


@pytest.mark.parametrize("name,B,T", [("small", 3, 160), ("full", 2, 1000)])
def test_moments_match_the_fp32_restatement(name, B, T):
    """All 2L channels before the clamp: relative L2 below 1e-2, the bound every network forward of the project is held to
    (tests/test_gpu_fullsize_parity.py)."""
    from diffmusic_amd.engine import VAE_DEFAULT
    eng, ref = _pair(SMALL if name == "small" else VAE_DEFAULT)
    mel = _mel(B, T)
    got = eng.encode_hip(mel)
    with torch.no_grad():
        want = ref(mel.cpu())
    s = eng.scale_factor
    assert got.shape == want.shape == (B, (T // s) * (64 // s), 16)
    r = _rel(got, want)
    print(f"vae encoder moments rel-L2 vs fp32 restatement ({name}, B={B}, T={T}): {r:.3e}")
    assert r < 1e-2
    d = eng.encode(mel).latent_dist
    L = 8
    want_nchw = want.reshape(B, T // s, 64 // s, 2 * L).permute(0, 3, 1, 2)
    assert _rel(d.mean, want_nchw[:, :L]) < 1e-2
    assert torch.equal(d.logvar, got.reshape(B, T // s, 64 // s, 2 * L).permute(0, 3, 1, 2)[:, L:].clamp(-30.0, 20.0))
    assert torch.equal(d.mode(), d.mean)


def test_limits_are_said_in_the_error():
    from diffmusic_amd import _lib
    from diffmusic_amd.engine import VaeEncoderEngine
    eng = VaeEncoderEngine(SMALL)
    eng.load_state_dict(eng.synth_state_dict(seed=1))
    with pytest.raises(_lib.DmxError, match="multiples of 2"):
        eng.encode_hip(torch.zeros(1, 162, 64, device="cuda"))
    with pytest.raises(_lib.DmxError, match="batch"):
        eng.encode_hip(torch.zeros(65, 16, 64, device="cuda"))


@pytest.mark.parametrize("B,Ci,Co,H,W", [(2, 32, 32, 32, 16), (2, 12, 20, 16, 16), (1, 64, 64, 40, 64)])
def test_asymmetric_pad_stride2_convolution_alone(B, Ci, Co, H, W):
    """The downsampler's descriptor (zero rows / columns after the image only) against F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2),
    through the layer builder every executor uses (dmx_conv2d_raw): W = 16 -> 8 and channel counts that need padding included."""
    from diffmusic_amd import _lib as L
    from diffmusic_amd._ctypes_ops import _p, _stream
    g = torch.Generator().manual_seed(B * 1000 + Ci)
    x = torch.randn(B, Ci, H, W, generator=g).to(L.act_dtype())
    w = torch.randn(Co, Ci, 3, 3, generator=g) / math.sqrt(9 * Ci)
    b = 0.1 * torch.randn(Co, generator=g)
    want = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w, b, stride=2)
    Cip, Cop = (Ci + 7) // 8 * 8, (Co + 7) // 8 * 8
    xin = torch.zeros(B, H, W, Cip, dtype=L.act_dtype())
    xin[..., :Ci] = x.permute(0, 2, 3, 1)
    xin = xin.cuda().contiguous()
    y = torch.full((B, H // 2, W // 2, Cop), float("nan"), dtype=L.act_dtype(), device="cuda")
    wc, bc = w.contiguous(), b.contiguous()
    L.check(L.lib().dmx_conv2d_raw(C.c_void_p(wc.data_ptr()), C.c_void_p(bc.data_ptr()), _p(xin), _p(y), B, H, W, Ci, Co, 3, 2, 0, 1,
                                   _stream()), "conv2d_raw")
    torch.cuda.synchronize()
    assert tuple(want.shape) == (B, Co, H // 2, W // 2)
    got = y[..., :Co].permute(0, 3, 1, 2).float().cpu()
    r = _rel(got, want)
    print(f"asymmetric-pad stride-2 conv rel-L2 (Ci={Ci}, Co={Co}, {H}x{W}): {r:.3e}")
    assert r < 1e-2
    assert float(y[..., Co:].float().abs().max()) == 0.0 if Cop > Co else True
    # the symmetric descriptor is untouched: the U-Net's stride-2 pad-1 sampler through the same hook
    y1 = torch.empty(B, H // 2, W // 2, Cop, dtype=L.act_dtype(), device="cuda")
    L.check(L.lib().dmx_conv2d_raw(C.c_void_p(wc.data_ptr()), C.c_void_p(bc.data_ptr()), _p(xin), _p(y1), B, H, W, Ci, Co, 3, 2, 1, 1,
                                   _stream()), "conv2d_raw")
    assert _rel(y1[..., :Co].permute(0, 3, 1, 2).float(), F.conv2d(x.float(), w, b, stride=2, padding=1)) < 1e-2


def test_batch_invariance_is_bit_exact():
    """Clip k of a B = 3 encode equals, bit for bit, the encode of that clip alone and at another batch position."""
    eng, _ = _pair(SMALL)
    mel = _mel(3, 160, seed=7)
    base = eng.encode_hip(mel).clone()
    for k in range(3):
        assert torch.equal(eng.encode_hip(mel[k:k + 1].contiguous())[0], base[k]), f"clip {k} alone"
    order = [2, 0, 1]
    perm = eng.encode_hip(mel[order].contiguous())
    for pos, k in enumerate(order):
        assert torch.equal(perm[pos], base[k]), f"clip {k} at position {pos}"


def test_batch_invariance_at_full_size():
    """The shapes users run (VAE_DEFAULT, 1000 frames): clip k of a B = 2 encode equals the clip encoded alone, bit for bit."""
    from diffmusic_amd.engine import VAE_DEFAULT
    eng, _ = _pair(VAE_DEFAULT)
    mel = _mel(2, 1000, seed=8)
    base = eng.encode_hip(mel).clone()
    for k in range(2):
        assert torch.equal(eng.encode_hip(mel[k:k + 1].contiguous())[0], base[k]), f"clip {k} alone"


@pytest.mark.parametrize("h,w", [(5, 16), (3, 5)])
def test_latent_init_against_the_torch_formula(h, w):
    """fp32 in, fp32 out, elementwise arithmetic: 1e-5 relative.  Covers eps = None (posterior mode), logvar outside [-30, 20], no noise
    term, and abar = the first and the last entry of the scheduler's table."""
    from diffmusic_amd import ops
    from diffmusic_amd.schedulers.scheduling_guided import GuidedDDIMScheduler
    from tests.stubs import SCHED
    ac = GuidedDDIMScheduler(**SCHED)._ac
    B, L, sf = 3, 8, 0.9227914214134216
    g = torch.Generator().manual_seed(h)
    mom = torch.randn(B, h * w, 2 * L, generator=g)
    mom[..., L:] *= 25.0                                         # logvar well outside the clamp on both sides
    assert float(mom[..., L:].max()) > 20.0 and float(mom[..., L:].min()) < -30.0
    eps, noise = torch.randn(B, L, h, w, generator=g), torch.randn(B, L, h, w, generator=g)
    nchw = mom.reshape(B, h, w, 2 * L).permute(0, 3, 1, 2)
    mean, logvar = nchw[:, :L], nchw[:, L:].clamp(-30.0, 20.0)
    md, ed, nd = mom.cuda(), eps.cuda(), noise.cuda()
    for abar in (float(ac[0]), float(ac[-1])):
        sa, s1 = abar ** 0.5, (1.0 - abar) ** 0.5
        for e, n in ((ed, nd), (None, nd), (ed, None), (None, None)):
            m, lv, x = ops.hip.latent_init(md, h, w, e, n, sa, sf, s1, True)
            z = mean if e is None else mean + torch.exp(0.5 * logvar) * eps
            want = sa * sf * z + (0.0 if n is None else s1 * noise)
            assert torch.equal(m.cpu(), mean) and torch.equal(lv.cpu(), logvar)
            assert _rel(x, want) < 1e-5, (abar, e is None, n is None)
    m, lv, x = ops.hip.latent_init(md, h, w, None, None, 1.0, 1.0, 0.0, False)
    assert x is None and torch.equal(m.cpu(), mean)


def test_both_bindings_are_bit_identical(monkeypatch):
    from diffmusic_amd import ops
    eng, _ = _pair(SMALL)
    mel = _mel(2, 160, seed=9)
    assert ops.enabled()
    a = eng.encode_hip(mel).clone()
    g = torch.Generator().manual_seed(1)
    eps, noise = torch.randn(2, 8, 40, 16, generator=g).cuda(), torch.randn(2, 8, 40, 16, generator=g).cuda()
    la = ops.hip.latent_init(a, 40, 16, eps, noise, 0.8, 0.92, 0.6, True)
    monkeypatch.setattr(ops, "USE_TORCH_OPS", False)
    assert not ops.enabled()
    b = eng.encode_hip(mel)
    lb = ops.hip.latent_init(b, 40, 16, eps, noise, 0.8, 0.92, 0.6, True)
    assert torch.equal(a, b)
    for u, v in zip(la, lb):
        assert torch.equal(u, v)


def test_model_mel_frontend_equals_its_float64_definition():
    """STFT magnitudes (n_fft 1024, hop 160, periodic hann, centred, reflect-padded) through the slaney mel bank, in float64, on a
    160 000-sample clip; the criterion of the operator's log-mel test (tests/test_gpu_parity_rows.py): every bin within 40 dB of the
    clip's strongest is within 1e-4 dB.  Frames are cropped, or padded with the floor, to the requested count."""
    import bench
    from diffmusic_amd.inverse_problem.operator import ModelMelFrontend
    length = 160000
    g = torch.Generator().manual_seed(5)
    wav = torch.stack([bench.synth_clip(0, length), 0.3 * torch.randn(length, generator=g)])
    fe = ModelMelFrontend()
    got = fe(wav.cuda().contiguous(), length, 1000).cpu().double()
    spec = torch.stft(wav.double(), 1024, 160, window=torch.hann_window(1024, periodic=True, dtype=torch.float64), center=True,
                      pad_mode="reflect", return_complex=True).abs()                        # (B, 513, 1001)
    truth = (spec.transpose(1, 2) @ torch.from_numpy(fe.fb).double())[:, :1000]
    assert got.shape == truth.shape == (2, 1000, 64)
    db_t, db_g = 20.0 * torch.log10(truth.clamp_min(1e-30)), 20.0 * torch.log10(got.clamp_min(1e-30))
    strong = db_t > db_t.amax(dim=(1, 2), keepdim=True) - 40.0
    err = (db_g - db_t).abs()
    print(f"model mel |err| dB vs float64 on strong bins: {float(err[strong].max()):.2e}")
    assert float(err[strong].max()) <= 1e-4
    padded = fe(wav.cuda().contiguous(), length, 1008)
    assert padded.shape == (2, 1008, 64) and torch.equal(padded[:, :1000].cpu().double(), got)
    assert torch.equal(padded[:, 1001:], torch.full_like(padded[:, 1001:], fe.log_floor))
    # the log is taken by the encoder's input stage: ln(max(x, floor)) on load equals encoding the log-mel itself
    eng, _ = _pair(SMALL)
    lin = padded[:, :160].contiguous()
    # (not bit-equal: the two logs may differ in the last fp32 bit, one flipped 16-bit rounding of an input re-rolls the 16-bit roundings of
    #  everything downstream, so the two results are two 16-bit evaluations of the same function: each is within the project's 1e-2 of the
    #  exact network, hence within 2e-2 of each other)
    assert _rel(eng.encode_hip(lin, log_floor=fe.log_floor), eng.encode_hip(torch.log(lin.clamp_min(fe.log_floor)))) < 2e-2
