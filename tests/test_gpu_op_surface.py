"""-m gpu: one op per operation (csrc_torch/torch_ops.cpp, diffmusic_amd/_ctypes_ops.py).  For every argument that an op takes beyond its
plain form, the torch op and the ctypes function of the same name return the same bits, and a call that omits the defaulted arguments
returns the bits of the call that passes the defaults.  Caller-owned results come back as the caller's storage with nothing written
outside it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CANARY = 12345.678
L_, PAD = 2208, 37                                # the fused STFT-mel path needs >= 2048 samples; 2208 is no multiple of the hop


def _bindings():
    from diffmusic_amd import ops
    return ops.load(), ops.ctypes_hip


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _strided(rows, n):
    """-> (buf (rows, n + PAD) of canaries, its row-strided view buf[:, :n])"""
    buf = torch.full((rows, n + PAD), CANARY, dtype=torch.float32, device="cuda")
    return buf, buf[:, :n]


def _intact(buf, n):
    return bool((buf[:, n:] == CANARY).all())


@pytest.fixture(scope="module")
def fe():
    from diffmusic_amd.inverse_problem.operator import SpectralFrontend
    return SpectralFrontend(16000, 1024, 160, 64, "hann")


# ---- scheduler arithmetic ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip_r", [0.0, 0.5])
@pytest.mark.parametrize("ptype", [0, 1, 2])
def test_sched_pred_x0_prediction_type_and_clip_range(ptype, clip_r):
    h, c = _bindings()
    x, e = _randn(2, 8, 5, 4, seed=1), _randn(2, 8, 5, 4, seed=2)
    a, b = h.sched_pred_x0(x, e, 0.37, ptype=ptype, clip_r=clip_r), c.sched_pred_x0(x, e, 0.37, ptype=ptype, clip_r=clip_r)
    assert _same(a, b) and bool(torch.isfinite(a).all())
    if clip_r:
        assert float(a.abs().max()) <= clip_r
    if ptype == 0 and clip_r == 0.0:
        for binding in (h, c):
            assert _same(binding.sched_pred_x0(x, e, 0.37), a)


@pytest.mark.parametrize("mode", [1, 3])
def test_sched_update_prediction_type_clip_range_and_grad_out(mode):
    h, c = _bindings()
    shp = (2, 8, 5, 4)
    x, e, g0, z = (_randn(*shp, seed=s) for s in range(4))
    inv = torch.rand(2, generator=torch.Generator().manual_seed(9)).cuda() + 0.5
    x0 = h.sched_pred_x0(x, e, 0.37, ptype=2, clip_r=0.5)
    args = (mode, x, e, x0, g0, inv, z if mode == 3 else None, 0.37, 0.41, 0.2, 0.08, 1e-8, False)
    outs = []
    for binding in (h, c):
        grad = torch.full(shp, float("nan"), device="cuda")
        prev, x0_out = binding.sched_update(*args, ptype=2, clip_r=0.5, grad_out=grad)
        assert x0_out is None and bool(torch.isfinite(prev).all()) and bool(torch.isfinite(grad).all())
        outs.append((prev, grad))
    assert _same(outs[0][0], outs[1][0]) and _same(outs[0][1], outs[1][1])
    for binding in (h, c):                                            # the defaults: omitted = passed, and both bindings agree
        p0, n0 = binding.sched_update(*args)
        p1, n1 = binding.sched_update(*args, ptype=0, clip_r=0.0, grad_out=None)
        assert _same(p0, p1) and n0 is None and n1 is None
        outs.append((p0,))
    assert _same(outs[2][0], outs[3][0]) and not _same(outs[2][0], outs[0][0])


# ---- the guidance pair -------------------------------------------------------------------------------------------------------------------
def test_mel_guidance_noise_and_threshold_combinations(fe):
    from diffmusic_amd import _lib
    h, c = _bindings()
    B, full = 2, L_ + 32
    T, bins = _lib.lib().dmx_audio_num_frames(fe._h, L_), _lib.lib().dmx_audio_num_bins(fe._h)
    wav = 0.3 * _randn(B, full, seed=3)
    ref = fe.transform_fwd(0.3 * _randn(B, full, seed=4), L_, False, False, -80.0, 80.0).clone()
    assert ref.shape == (B, T, 64) and fe.fused(L_)
    st = fe._get_state(B, L_, wav.device)
    noise, noise_mag = _randn(B, full, seed=5), _randn(B, bins, T, seed=6)
    thr = torch.tensor([0.2, 0.35], device="cuda")
    args = (fe._h.value, wav, None, ref, st, L_, full, False, False, -80.0, 80.0, 0.5)
    seen = []
    for n in (None, noise):
        for m in (None, noise_mag):
            for t in (None, thr):
                a, b = h.mel_guidance(*args, n, m, 0.05, t), c.mel_guidance(*args, n, m, 0.05, t)
                assert _same(a[0], b[0]) and _same(a[1], b[1]), (n is None, m is None, t is None)
                assert a[0].shape == (B,) and a[1].shape == (B, full) and bool((a[1][:, L_:] == 0).all())
                assert all(not _same(a[1], s) for s in seen)           # every operand changes the result
                seen.append(a[1])
    for binding in (h, c):
        plain = binding.mel_guidance(*args)
        given = binding.mel_guidance(*args, None, None, 0.0, None)
        assert _same(plain[0], given[0]) and _same(plain[1], given[1]) and _same(plain[1], seen[0])


# ---- caller-owned results ---------------------------------------------------------------------------------------------------------------
def test_logmel_caller_owned_results(fe):
    from diffmusic_amd import _lib
    B = 2
    T = _lib.lib().dmx_audio_num_frames(fe._h, L_)
    wav, dmel = 0.3 * _randn(B, L_ + 32, seed=7), _randn(B, T, 64, seed=8)
    st = fe._get_state(B, L_, wav.device)
    flags = (L_, True, True, -80.0, 80.0)
    res = []
    for binding in _bindings():
        mel = binding.logmel_fwd(fe._h.value, wav, st, *flags)
        # dmx_audio_transform_fwd takes no row stride for the mel: the caller-owned form is a contiguous window of a wider buffer
        buf = torch.full((B * T * 64 + PAD,), CANARY, dtype=torch.float32, device="cuda")
        view = buf[:B * T * 64].view(B, T, 64)
        got = binding.logmel_fwd(fe._h.value, wav, st, *flags, out=view)
        assert got.data_ptr() == view.data_ptr() and _same(view, mel) and bool((buf[B * T * 64:] == CANARY).all())
        with pytest.raises((RuntimeError, AssertionError)):
            binding.logmel_fwd(fe._h.value, wav, st, *flags, out=torch.empty(B, T, 64 + PAD, device="cuda")[:, :, :64])
        d = binding.logmel_bwd(fe._h.value, dmel, st, *flags)
        wide, dview = _strided(B, L_)
        got = binding.logmel_bwd(fe._h.value, dmel, st, *flags, dwav=dview)
        assert d.shape == (B, L_) and got.data_ptr() == dview.data_ptr() and got.stride(0) == L_ + PAD
        assert _same(dview, d) and _intact(wide, L_)
        res.append((mel, d))
    assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1])


def test_stft_mag_bwd_caller_owned_result(fe):
    from diffmusic_amd import _lib
    B = 2
    T, bins = _lib.lib().dmx_audio_num_frames(fe._h, L_), _lib.lib().dmx_audio_num_bins(fe._h)
    wav, dmag = 0.3 * _randn(B, L_ + 32, seed=10), _randn(B, bins, T, seed=11)
    st = fe._get_state(B, L_, wav.device)
    res = []
    for binding in _bindings():
        binding.stft_mag_fwd(fe._h.value, wav, st, L_)
        d = binding.stft_mag_bwd(fe._h.value, dmag, st, L_, L_ + 32)
        assert d.shape == (B, L_ + 32) and bool((d[:, L_:] == 0).all())
        wide, view = _strided(B, L_)
        got = binding.stft_mag_bwd(fe._h.value, dmag, st, L_, L_, dwav=view)
        assert got.data_ptr() == view.data_ptr() and _same(view, d[:, :L_]) and _intact(wide, L_)
        res.append(d)
    assert _same(res[0], res[1])


def test_tf_gain_caller_owned_result(fe):
    from diffmusic_amd import _lib
    B = 2
    T = _lib.lib().dmx_audio_tf_frames(L_)
    x = 0.3 * _randn(B, L_ + 32, seed=12)
    gain = torch.rand(B, T, 513, generator=torch.Generator().manual_seed(13)).cuda()
    res = []
    for binding in _bindings():
        y = binding.tf_gain(fe._h.value, x, gain, L_, L_)
        wide, view = _strided(B, L_)
        got = binding.tf_gain(fe._h.value, x, gain, L_, L_, out=view)
        assert got.data_ptr() == view.data_ptr() and _same(view, y) and _intact(wide, L_)
        res.append(y)
    assert _same(res[0], res[1])


def test_l2norm_without_the_gradient():
    ref, pred = _randn(2, 14, 64, seed=14), _randn(2, 14, 64, seed=15)
    res = []
    for binding in _bindings():
        loss, dpred = binding.l2norm(ref, pred, 0.5)
        loss2, none = binding.l2norm(ref, pred, 0.5, want_grad=False)
        loss3, dpred3 = binding.l2norm(ref, pred, 0.5, want_grad=True)
        assert none is None and _same(loss, loss2) and _same(loss, loss3) and _same(dpred, dpred3) and dpred.shape == pred.shape
        res.append((loss, dpred))
    assert _same(res[0][0], res[1][0]) and _same(res[0][1], res[1][1])


# ---- networks ---------------------------------------------------------------------------------------------------------------------------
def test_hifigan_fwd_span_arguments():
    from diffmusic_amd import _lib
    from diffmusic_amd.engine import HifiGanEngine
    from tests.test_gpu_step import HIFI
    h, c = _bindings()
    voc = HifiGanEngine(HIFI)
    voc.load_state_dict(voc.synth_state_dict(1))
    mel = torch.randn(2, 40, 64, generator=torch.Generator().manual_seed(2)).to(_lib.act_dtype()).cuda()
    plain = voc.forward(mel).clone()                                  # (sizes the workspace)
    ws, m = voc._ws["buf"], voc._h.value
    n = plain.shape[1]
    for binding in (h, c):
        for span in ((), (0, 0), (5, 5)):                             # an empty span is the plain forward
            assert _same(binding.hifigan_fwd(m, mel, ws, *span), plain), span
    s0, s1 = n // 4, 3 * n // 4                                       # a real hole: the same bits and the same plan in both bindings
    stages = len(HIFI["upsample_rates"])
    a = h.hifigan_fwd(m, mel, ws, s0, s1).clone()
    plan = list(h.hifigan_dead_plan(m, stages))
    b = c.hifigan_fwd(m, mel, ws, s0, s1)
    assert _same(a, b) and c.hifigan_dead_plan(m, stages) == plan
    assert _same(a[:, :s0], plain[:, :s0]) and _same(a[:, s1:], plain[:, s1:])
    # a span that saves a whole slab of rows somewhere comes back as zeros; one too short for that is the plain forward
    assert bool((a[:, s0:s1] == 0).all()) if sum(plan[0::4]) > 0 else _same(a, plain)


def _unet(cfg, seed):
    from diffmusic_amd.engine import UNetEngine
    un = UNetEngine(cfg)
    un.load_state_dict(un.synth_state_dict(seed))
    return un


def test_unet_fwd_context_and_output_channels():
    from tests.test_gpu_unet import SMALL
    h, c = _bindings()
    x, t, cls = _randn(2, 8, 26, 16, seed=20), torch.full((2,), 501.0).cuda(), _randn(2, 512, seed=21)
    un = _unet(SMALL, 9)
    eps = un.forward(x, t, cls).clone()                               # (sizes the workspace)
    ws, m = un._ws["buf"], un._h.value
    for binding in (h, c):
        assert _same(binding.unet_fwd(m, x, t, cls, ws), eps)
        assert _same(binding.unet_fwd(m, x, t, cls, ws, None, None, None, out_channels=None), eps)
        assert _same(binding.unet_fwd(m, x, t, cls, ws, out_channels=8), eps)
    # the two context streams of the AudioLDM2 U-Net
    a2 = _unet(dict(SMALL, class_embed_dim=0, attn_cross_dims=[0, 48, 64]), 3)
    c0, c1 = _randn(2, 8, 48, seed=22), _randn(2, 12, 64, seed=23)
    m1 = torch.ones(2, 12).cuda()
    m1[1, 9:] = 0
    eps2 = a2.forward(x, t, None, c0, c1, m1).clone()
    bias1 = ((1.0 - m1) * -10000.0).contiguous()
    ws2, m2 = a2._ws["buf"], a2._h.value
    for binding in (h, c):
        assert _same(binding.unet_fwd(m2, x, t, None, ws2, c0, c1, bias1), eps2)
        for some in ((c0, None, None), (c0, c1, None), (None, c1, bias1), (None, None, bias1)):
            with pytest.raises(RuntimeError, match="all three or none"):
                binding.unet_fwd(m2, x, t, None, ws2, *some)
    assert not _same(eps2, eps)
    # a U-Net whose output channels differ from its input's
    u4 = _unet(dict(SMALL, out_channels=4), 5)
    eps4 = u4.forward(x, t, cls).clone()
    ws4, m4 = u4._ws["buf"], u4._h.value
    assert eps4.shape == (2, 4, 26, 16) and bool(torch.isfinite(eps4).all()) and float(eps4.abs().max()) > 0
    for binding in (h, c):
        got = binding.unet_fwd(m4, x, t, cls, ws4, out_channels=4)
        assert got.shape == (2, 4, 26, 16) and _same(got, eps4)


# ---- Philox seeds beyond the signed range -------------------------------------------------------------------------------------------------
def test_randn_philox_folds_64_bit_seeds():
    from diffmusic_amd import ops
    from diffmusic_amd.torch_utils import randn_philox
    seeds, shape = [2 ** 63, 2 ** 64 - 1, 7], (3, 1, 5, 7)
    for offset in (0, 2 ** 63 + 3):
        a = randn_philox(shape, seeds, offset, "cuda")
        b = ops.ctypes_hip.randn_philox(shape, seeds, offset, torch.device("cuda"))
        assert _same(a, b) and bool(torch.isfinite(a).all())
    assert not _same(a[0], a[1]) and not _same(a[0], randn_philox(shape, [0, 1, 7], 0, "cuda")[0])
