"""-m gpu: time-frequency masking (csrc/tf_gain.hip, inverse_problem/operator.py TimeFrequencyMaskOperator).

Kernel level: every case of tests/tf_gain_cases.py against the float64 model, EVERY element within the bound derived from the number
formats, through both bindings (bit-identical); identity, the adjoint identity under the same bound, reproducibility and layout, refusals
through the C ABI.  Operator level: the contract of tests/test_gpu_operator_contract.py for the new operator, the dead span.  Step level:
teacher-forced steps against `oracle.schedulers` around `OracleTF` below -- a torch fp32 restatement of A from torch.fft.rfft / irfft on
explicitly framed, zero-extended input wrapped around the oracle IdentityOperator's transform -- with the bounds of tests/test_gpu_step.py;
inside a TrackOperator and a MixtureOperator against their oracle wrappers.  Call level: `pipe(...)` equals a hand-written loop bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import tf_gain_cases as TF                                                  # noqa: E402
from tests.test_gpu_step import HIFI, VAE, SCHED, H, W as LAT_W, LEN                   # noqa: E402

CANARY = 12345.678
_REPORT = {}


@pytest.fixture(scope="module")
def fe():
    from diffmusic_amd.inverse_problem.operator import SpectralFrontend
    return SpectralFrontend(16000, 1024, 160, 64, "hann")


def _bindings():
    from diffmusic_amd import ops
    return (("torch_ops", ops.load()), ("ctypes", ops.ctypes_hip))


def _dev_case(c):
    i = TF.inputs(c)
    store = torch.from_numpy(i.store).cuda()                       # (B, stride): clip b at row b
    x = store[:, :c.full]
    gt = torch.from_numpy(np.ascontiguousarray(np.swapaxes(i.gain, -1, -2))).cuda()
    return i, x, gt


def _bits(t):
    return t.contiguous().view(torch.int32)


def _canary_out(B, full, stride, slack=64):
    buf = torch.full((B * stride + slack,), CANARY, dtype=torch.float32, device="cuda")
    return buf, buf[:B * stride].view(B, stride)[:, :full]


def _untouched_outside(buf, B, full, stride):
    keep = torch.ones(buf.numel(), dtype=torch.bool, device="cuda")
    for b in range(B):
        keep[b * stride: b * stride + full] = False
    return bool((buf[keep] == CANARY).all())


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TF.CASES, ids=lambda c: c.name)
def test_kernel_lies_within_the_bound_in_every_element(fe, c):
    from diffmusic_amd import ops
    i, x, gt = _dev_case(c)
    r, q = TF.reference(c)
    h = fe._h.value
    outs = []
    for name, binding in _bindings():
        out = binding.tf_gain(h, x, gt, c.L, c.full)
        assert out.shape == (c.B, c.full) and out.is_contiguous()
        ratio = TF.ratio(out[:, :c.L].cpu().numpy(), r.y, q)
        _REPORT[c.name] = max(_REPORT.get(c.name, 0.0), ratio)
        print(f"\n  {c.name}/{name}: largest |kernel - model| / bound = {ratio:.4f}")
        assert ratio <= 1.0, (c.name, name, ratio)
        assert bool((_bits(out[:, c.L:]) == 0).all()), "out[:, L:full] is +0.0f"
        if c.gain == "ones":                                       # identity: |A x - x| <= bound, element-wise
            assert TF.ratio(out[:, :c.L].cpu().numpy(), i.x.astype(np.float64), q) <= 1.0, c.name
        outs.append(out)
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "the two bindings are bit-identical"
    # caller-owned strided output: nothing past `full`, or past a row's stride, is written
    buf, view = _canary_out(c.B, c.full, c.out_stride)
    got = ops.ctypes_hip.tf_gain(h, x, gt, c.L, c.full, out=view)
    assert got.data_ptr() == view.data_ptr() and torch.equal(_bits(view), _bits(outs[0]))
    assert _untouched_outside(buf, c.B, c.full, c.out_stride)


@pytest.mark.parametrize("name", ["L300_rand", "L2049_rand_pc", "L4999_rand_pc", "L6400_zero_frames"])
def test_the_kernel_is_its_own_transpose(fe, name):
    """|<A x, y> - <x, A y>| <= sum |y| b(A x) + sum |x| b(A y): float64 accumulation of the fp32 outputs, the element-wise bound"""
    from diffmusic_amd import ops
    c = TF.CASE[name]
    i, x, gt = _dev_case(c)
    y64 = 0.3 * np.random.default_rng(7).standard_normal((c.B, c.L))
    y32 = y64.astype(np.float32)
    yd = torch.from_numpy(y32).cuda()
    Ax = ops.hip.tf_gain(fe._h.value, x, gt, c.L, c.L).cpu().numpy().astype(np.float64)
    Ay = ops.hip.tf_gain(fe._h.value, yd, gt, c.L, c.L).cpu().numpy().astype(np.float64)
    _, bAx = TF.reference(c)
    ry = TF.model(y32, i.gain, c.L)
    bAy = TF.bound(y32, i.gain, c.L, ry)
    xs, ys = i.x.astype(np.float64), y32.astype(np.float64)
    for b in range(c.B):
        lhs, rhs = float(Ax[b] @ ys[b]), float(xs[b] @ Ay[b])
        tol = float(np.abs(ys[b]) @ bAx[b] + np.abs(xs[b]) @ bAy[b])
        print(f"\n  {name}[{b}]: <Ax, y> = {lhs:.9g}, <x, Ay> = {rhs:.9g}, |difference| = {abs(lhs - rhs):.3g} <= {tol:.3g}")
        assert abs(lhs - rhs) <= tol, (name, b, lhs, rhs, tol)


def test_reproducibility_and_layout(fe):
    from diffmusic_amd import ops
    h = fe._h.value
    for name in ("L4999_rand_pc", "L6400_stride", "L2049_rand"):
        c = TF.CASE[name]
        i, x, gt = _dev_case(c)
        first = ops.hip.tf_gain(h, x, gt, c.L, c.full)
        assert torch.equal(_bits(first), _bits(ops.hip.tf_gain(h, x, gt, c.L, c.full))), "two runs are bit-equal"
        for b in range(c.B):                                       # a clip alone = the clip at position b of the batch
            g_b = gt[b] if c.per_clip else gt
            alone = ops.hip.tf_gain(h, x[b:b + 1], g_b, c.L, c.full)
            assert torch.equal(_bits(alone[0]), _bits(first[b])), (name, b)
        swapped = ops.hip.tf_gain(h, x.flip(0).contiguous(), gt.flip(0).contiguous() if c.per_clip else gt, c.L, c.full)
        assert torch.equal(_bits(swapped.flip(0)), _bits(first)), "batch position does not matter"
        if not c.per_clip:                                         # a shared grid = the same grid repeated per clip
            rep = gt[None].expand(c.B, -1, -1).contiguous()
            assert torch.equal(_bits(ops.hip.tf_gain(h, x, rep, c.L, c.full)), _bits(first)), name
    c = TF.CASE["L6400_stride"]
    assert c.full > c.L and c.stride > c.full


def test_refusals_through_the_c_abi_write_nothing(fe):
    from diffmusic_amd import _lib
    from diffmusic_amd.inverse_problem.operator import SpectralFrontend
    lib = _lib.lib()
    L, full, B = 1500, 1510, 2
    T = lib.dmx_audio_tf_frames(L)
    assert T == TF.frames(L) and lib.dmx_audio_tf_frames(0) == 0
    x = torch.randn(B, full, device="cuda")
    g = torch.ones(T, 513, device="cuda")
    rect = SpectralFrontend(16000, 1024, 160, 64, "rect")
    short = SpectralFrontend(16000, 512, 160, 64, "hann")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(handle, xs=full, gs=0, os_=full, L_=L, full_=full, xp=x.data_ptr(), gp=g.data_ptr(), out_null=False):
        buf, view = _canary_out(B, full, full)
        rc = lib.dmx_audio_tf_gain(handle, C.c_void_p(xp), xs, C.c_void_p(gp), gs, C.c_void_p(0 if out_null else view.data_ptr()), os_, B, L_,
                                   full_, st)
        torch.cuda.synchronize()
        return rc, bool((buf == CANARY).all())
    ok = fe._h
    assert call(ok) == (0, False)                                  # the same call with nothing wrong runs
    for what, kw in (("rectangular window", dict(handle=rect._h)), ("n_fft 512", dict(handle=short._h)), ("full < L", dict(full_=L - 1)),
                     ("short x stride", dict(xs=L - 1)), ("short out stride", dict(os_=full - 1)), ("L < 1", dict(L_=0)),
                     ("short gain stride", dict(gs=T * 513 - 1)), ("null x", dict(xp=0)), ("null gain", dict(gp=0)), ("null out", dict(out_null=True)),
                     ("null handle", dict(handle=C.c_void_p(0)))):
        rc, untouched = call(kw.pop("handle", ok), **kw)
        assert rc != 0 and untouched, what
        assert lib.dmx_last_error(), what
    from diffmusic_amd import ops
    for _, binding in _bindings():                                 # and the bindings' own checks
        with pytest.raises((RuntimeError, AssertionError)):
            binding.tf_gain(ok.value, x, g[:-1].contiguous(), L, full)
        with pytest.raises((RuntimeError, AssertionError)):
            binding.tf_gain(ok.value, x, g, L, L - 1)
        with pytest.raises((RuntimeError, AssertionError)):
            binding.tf_gain(rect._h.value, x, g, L, full)
    assert ops.hip.tf_gain(ok.value, x, g, L, full).shape == (B, full)


def test_report_largest_ratios():
    if _REPORT:
        worst = max(_REPORT, key=_REPORT.get)
        print(f"\n  largest |kernel - model| / bound over {len(_REPORT)} cases: {_REPORT[worst]:.4f} ({worst})")


# ---- operator level: the contract ---------------------------------------------------------------------------------------------------------
def _grid(length, per_clip=False, seed=0):
    """a band-stop box, a spectral hole and a smooth random part, so that no bin or frame is special"""
    from diffmusic_amd.inverse_problem import tf_gain_grid, tf_frames
    T = tf_frames(length)
    dur = length / 16000.0
    rng = np.random.default_rng(seed)
    grids = []
    for b in range(2 if per_clip else 1):
        g = tf_gain_grid(length, 16000, [(1000.0, 1500.0, None, None, 0.0), (3000.0, 5000.0, 0.3 * dur, 0.6 * dur, 0.0)]) \
            * rng.uniform(0.5, 1.5, (513, T)).astype(np.float32)
        grids.append(g)
    return np.stack(grids) if per_clip else grids[0]


def _tf_op(length, per_clip=False, noiser=None):
    from diffmusic_amd import inverse_problem as P
    return P.TimeFrequencyMaskOperator(16000, _grid(length, per_clip), noiser=noiser)


@pytest.mark.parametrize("per_clip", [False, True], ids=["shared", "per_clip"])
def test_guidance_is_the_composition_of_its_parts(per_clip, monkeypatch):
    """tests/test_gpu_operator_contract.py for the new operator: `guidance` = apply -> noise_add -> fused pair (2048) or dense chain (1600)
    -> adjoint, bit for bit, both spaces, with and without an injected noise at sigma = 0.05, in both bindings."""
    from diffmusic_amd import inverse_problem as P, ops
    from tests.test_gpu_operator_contract import B, PAD, SIGMA, _wave, _chain
    for length in (2048, 1600):
        op = _tf_op(length, per_clip)
        assert op._on_load(None, length) is None
        wav, clean = _wave(1, length + PAD, 0.05), _wave(2, length, 0.083)
        meas = op.forward(clean)
        assert meas.shape == (B, length)
        z = torch.randn(B, length, generator=torch.Generator().manual_seed(3)).cuda()
        for space in ("wav_form", "mel_spectrogram"):
            for sigma in (0.0, SIGMA):
                case = (per_clip, length, space, sigma)
                op.noiser = P.GaussianNoise(sigma)
                noise = z if sigma > 0 else None
                loss, dwav = op.guidance(wav, length, meas, space, noise=noise)
                assert loss.shape == (B,) and dwav.shape == wav.shape and bool(torch.isfinite(dwav).all()), case
                assert float(loss.min()) > 0 and float(dwav[:, length:].abs().max()) == 0.0 and float(dwav.abs().max()) > 0, case
                l2, d2 = _chain(op, wav, length, meas, space, noise, {}, fused_pair_on_y=True)
                assert torch.equal(loss, l2) and torch.equal(dwav, d2), case
                monkeypatch.setattr(ops, "USE_TORCH_OPS", False)   # the other binding: the same bits
                assert not ops.enabled()
                l3, d3 = op.guidance(wav, length, meas, space, noise=noise)
                monkeypatch.setattr(ops, "USE_TORCH_OPS", True)
                assert torch.equal(loss, l3) and torch.equal(dwav, d3), case
        op.noiser = P.GaussianNoise(0.0)
        assert torch.equal(op.forward(clean), op.apply(clean, length)[0])          # forward is apply plus the noiser
        fixed = torch.randn(B, length, generator=torch.Generator().manual_seed(4)).cuda()
        op.noiser = lambda y: y + 0.1 * fixed
        assert torch.equal(op.forward(clean), op.apply(clean, length)[0] + 0.1 * fixed)
        with pytest.raises(ValueError, match="513"):
            op.forward(_wave(9, length + 256, 0.05))
        with pytest.raises(ValueError, match="513"):
            op.guidance(_wave(9, length + 300, 0.05), length + 256, meas, "wav_form")


def test_the_transpose_is_a_transpose_and_is_stateless():
    from tests.test_gpu_operator_contract import B, PAD, _wave, _dot
    length = 2048
    op = _tf_op(length)
    x = _wave(4, length + PAD, 0.05)
    y, adjoint = op.apply(x, length)
    w = (y + 0.5 * torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).cuda()).contiguous()
    xt = adjoint(w, length + PAD).clone()
    assert xt.shape == x.shape and float(xt[:, length:].abs().max()) == 0.0
    lhs, rhs = _dot(y, w), _dot(x, xt)
    assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    y2, adjoint2 = op.apply(_wave(6, length + PAD, 0.11), length)                     # a later apply on another input
    assert torch.equal(adjoint(w, length + PAD), xt)
    assert adjoint2(y2, length + PAD).shape == (B, length + PAD)
    assert torch.equal(xt[:, :length], op.apply(w, length)[0])                        # A^T = A


# ---- step level -----------------------------------------------------------------------------------------------------------------------
def torch_tf(x, gain):
    """A in torch fp32, differentiable: x (B, L), gain (513, T) or (B, 513, T) -> (B, L).  Explicit zero extension and framing, rfft,
    gain, irfft, window, overlap-add by fold, 1 / 1.5."""
    B, L = x.shape
    T = gain.shape[-1]
    assert T == -(-L // 256) + 3
    total = (T - 1) * 256 + 1024
    w = torch.hann_window(1024, periodic=True, dtype=x.dtype)
    xp = torch.nn.functional.pad(x, (768, total - 768 - L))
    fr = xp.unfold(-1, 1024, 256)                                  # (B, T, 1024): frame t starts at sample (t - 3) * 256
    Y = torch.fft.rfft(fr * w, dim=-1) * gain.to(x.dtype).transpose(-1, -2)
    f = torch.fft.irfft(Y, n=1024, dim=-1) * w
    out = torch.nn.functional.fold(f.transpose(1, 2), output_size=(1, total), kernel_size=(1, 1024), stride=(1, 256))
    return out.reshape(B, total)[:, 768:768 + L] / 1.5


class OracleTF:
    """The oracle-side operator: forward = noiser(torch_tf(x)); transform / inverse_transform are the oracle IdentityOperator's."""

    def __init__(self, gain, noiser=None):
        from oracle import operators as O
        self.inner, self.gain, self.noiser = O.IdentityOperator(16000), torch.as_tensor(gain), noiser

    def forward(self, data, **k):
        y = torch_tf(data, self.gain)
        return self.noiser(y) if self.noiser is not None else y

    def transform(self, a):
        return self.inner.transform(a)

    def inverse_transform(self, mel, vocoder):
        return self.inner.inverse_transform(mel, vocoder)


class _FixedNoiser:
    def __init__(self, sigma, z):
        self.sigma, self.z = sigma, z

    def __call__(self, data):
        return data + self.sigma * self.z


def test_torch_restatement_agrees_with_the_float64_model():
    c = TF.CASE["L4999_rand_pc"]
    i = TF.inputs(c)
    r, _ = TF.reference(c)
    got = torch_tf(torch.from_numpy(i.x.copy()).double(), torch.from_numpy(i.gain).double()).numpy()
    assert np.abs(got - r.y).max() <= 1e-11 * max(1.0, np.abs(r.y).max())


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


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-300))


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.double().cpu().flatten(), b.double().cpu().flatten(), dim=0).item()


def _step_grid(T_samples):
    """a band-stop box (2 - 3 kHz, the whole clip) and a spectral hole (500 - 1500 Hz over the middle fifth)"""
    from diffmusic_amd.inverse_problem import tf_gain_grid
    dur = T_samples / 16000.0
    return tf_gain_grid(T_samples, 16000, [(2000.0, 3000.0, None, None, 0.0), (500.0, 1500.0, 0.4 * dur, 0.6 * dur, 0.0)])


STEP_CASES = [("dps", 0.0, 5e-4, "mel_spectrogram", 501, True, 0.0), ("dps", 0.0, 5e-4, "wav_form", 996, True, 0.0),
              ("mpgd", 0.0, 5e-3, "mel_spectrogram", 251, True, 0.0), ("dsg", 1.0, 0.08, "mel_spectrogram", 501, True, 0.0),
              ("dps", 0.0, 5e-4, "mel_spectrogram", 501, True, 0.05), ("dps", 0.0, 5e-4, "mel_spectrogram", 501, False, 0.0)]


def _compare(tag, sched, out, ro, name):
    rp, rl = _rel(out.prev_sample, ro.prev_sample), _rel(out.loss.reshape(-1), ro.loss.reshape(-1))
    cos = _cos(sched.last_grad, ro.sample)
    msg = f"{tag}: prev {rp:.2e} loss {rl:.2e} grad {_rel(sched.last_grad, ro.sample):.2e} cos {cos:.4f}"
    print("\n  " + msg)
    assert _rel(out.pred_original_sample, ro.pred_original_sample) < 1e-4 or name == "mpgd"
    assert rl < 1e-2, msg
    assert cos > 0.98, msg
    assert rp < 1e-2, msg


@pytest.mark.parametrize("name,eta,rate,space,t,per_clip,sigma", STEP_CASES,
                         ids=[f"{c[0]}-{c[3]}-{'clip' if c[5] else 'batch'}-sigma{c[6]}" for c in STEP_CASES])
def test_teacher_forced_step(nets, name, eta, rate, space, t, per_clip, sigma):
    """`_teacher_forced` of tests/test_gpu_step.py with the new operator: same x_t, eps and noise on both sides; forward rel-L2 < 1e-4,
    prev_sample <= 1e-2, loss <= 1e-2, gradient cosine > 0.98."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    from oracle import schedulers as OS
    voc, vae, rvoc, rvae = nets
    B = 2
    g = torch.Generator().manual_seed(77)
    clean = 0.3 * torch.sin(torch.arange(LEN) * 0.05)[None] * torch.tensor([[1.0], [0.6]]) + 0.05 * torch.randn(B, LEN, generator=g)
    x = torch.randn(B, 8, H, LAT_W, generator=g)
    e = torch.randn(B, 8, H, LAT_W, generator=g)
    z = torch.randn(B, 8, H, LAT_W, generator=g)
    z_meas, z_step = torch.randn(B, LEN, generator=g), torch.randn(B, LEN, generator=g)
    grid = _step_grid(LEN)
    op, rop = P.TimeFrequencyMaskOperator(16000, grid), OracleTF(grid)
    y_clean = rop.forward(clean)
    rf = _rel(op.forward(clean.cuda()), y_clean)
    print(f"\n  operator.forward rel-L2 {rf:.2e}")
    assert rf < 1e-4, "operator.forward"
    y_ref = y_clean + sigma * z_meas if sigma > 0 else y_clean
    y = y_ref.cuda() if sigma > 0 else op.forward(clean.cuda())
    op.noiser = P.GaussianNoise(sigma)
    rop.noiser = _FixedNoiser(sigma, z_step) if sigma > 0 else None
    sched = get_scheduler(name)(operator=op, per_clip_norm=per_clip, **SCHED)
    sched.set_timesteps(200)
    sched.debug_keep_grad = True
    rs = OS.get_scheduler(name)(operator=rop, per_clip_norm=per_clip, **SCHED)
    rs.set_timesteps(200)
    kw = dict(eta=eta, ip_guidance_rate=rate, original_waveform_length=LEN, supervised_space=space)
    noise_kw = dict(sample_noise=z.cuda()) if name == "dsg" else dict(variance_noise=None)
    opk = dict(noise=z_step.cuda()) if sigma > 0 else {}
    out = sched.step(e.cuda(), t, x.cuda(), measurement=y, vae=vae, vocoder=voc, op_kwargs=opk, **kw, **noise_kw)
    torch.cuda.synchronize()
    ro = rs.step(e, t, x, measurement=y_ref, vae=rvae, vocoder=rvoc, **kw, **(dict(sample_noise=z) if name == "dsg" else dict(variance_noise=None)))
    _compare(f"tf_mask {name}/{space}/{'clip' if per_clip else 'batch'}/sigma={sigma}", sched, out, ro, name)


def test_teacher_forced_track_step(nets):
    """One TrackOperator(TimeFrequencyMaskOperator) step at the (3, 6400, 1600, 16000) layout of tests/test_gpu_track.py, the gain built
    for the track's length, against OracleTrack(OracleTF)."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    from oracle import schedulers as OS
    from tests.test_gpu_track import OracleTrack, T3, R3, _clean_track
    voc, vae, rvoc, rvae = nets
    lay = P.TrackLayout(T3, LEN, R3)
    Wn = lay.num_windows
    assert Wn == 3
    grid = _step_grid(T3)
    op, rop = P.TimeFrequencyMaskOperator(16000, grid), OracleTF(grid)
    clean, g = _clean_track(T3)
    x = torch.randn(Wn, 8, H, LAT_W, generator=g)
    e = torch.randn(Wn, 8, H, LAT_W, generator=g)
    y_ref = rop.forward(clean)
    y = op.forward(clean.cuda())
    assert _rel(y, y_ref) < 1e-4, "operator.forward at track length"
    kw = dict(eta=0.0, ip_guidance_rate=5e-4, original_waveform_length=LEN, supervised_space="mel_spectrogram", variance_noise=None)
    rs = OS.get_scheduler("dps")(operator=OracleTrack(rop, lay), per_clip_norm=False, **SCHED)
    rs.set_timesteps(200)
    ro = rs.step(e, 501, x, measurement=y_ref, vae=rvae, vocoder=rvoc, **kw)
    sched = get_scheduler("dps")(operator=P.TrackOperator(op, lay), per_clip_norm=False, **SCHED)
    sched.set_timesteps(200)
    sched.debug_keep_grad = True
    out = sched.step(e.cuda(), 501, x.cuda(), measurement=y, vae=vae, vocoder=voc, **kw)
    torch.cuda.synchronize()
    assert out.loss.numel() == 1
    _compare("tf_mask inside a track", sched, out, ro, "dps")
    assert all(float(sched.last_grad[w].abs().max()) > 0 for w in range(Wn))


def test_teacher_forced_mixture_step(nets):
    """One MixtureOperator(TimeFrequencyMaskOperator, 2) step at LEN = 6400 against OracleMixture(OracleTF)."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    from oracle import schedulers as OS
    from tests.test_gpu_mixture import OracleMixture
    voc, vae, rvoc, rvae = nets
    K, gains = 2, (2.0, 0.5)
    grid = _step_grid(LEN)
    op, rop = P.TimeFrequencyMaskOperator(16000, grid), OracleTF(grid)
    g = torch.Generator().manual_seed(77)
    clean = 0.3 * torch.sin(torch.arange(LEN) * 0.05)[None] * torch.tensor([[1.0], [0.6]]) + 0.05 * torch.randn(K, LEN, generator=g)
    x = torch.randn(K, 8, H, LAT_W, generator=g)
    e = torch.randn(K, 8, H, LAT_W, generator=g)
    top, rtop = P.MixtureOperator(op, K, list(gains)), OracleMixture(rop, gains)
    y_ref = rtop.forward(clean)
    y = top.forward(clean.cuda())
    assert y_ref.shape[0] == 1 and _rel(y, y_ref) < 1e-4, "MixtureOperator.forward"
    kw = dict(eta=0.0, ip_guidance_rate=5e-4, original_waveform_length=LEN, supervised_space="mel_spectrogram", variance_noise=None)
    rs = OS.get_scheduler("dps")(operator=rtop, per_clip_norm=False, **SCHED)
    rs.set_timesteps(200)
    ro = rs.step(e, 501, x, measurement=y_ref, vae=rvae, vocoder=rvoc, **kw)
    sched = get_scheduler("dps")(operator=top, per_clip_norm=False, **SCHED)
    sched.set_timesteps(200)
    sched.debug_keep_grad = True
    out = sched.step(e.cuda(), 501, x.cuda(), measurement=y, vae=vae, vocoder=voc, **kw)
    torch.cuda.synchronize()
    assert out.loss.numel() == 1
    _compare("tf_mask inside a mixture", sched, out, ro, "dps")
    assert all(float(sched.last_grad[k].abs().max()) > 0 for k in range(K))


# ---- dead span ------------------------------------------------------------------------------------------------------------------------------
def _dead_grid():
    from diffmusic_amd.inverse_problem import tf_gain_grid
    return tf_gain_grid(LEN, 16000, [(2000.0, 3000.0, None, None, 0.0), (None, None, 0.1, 0.25, 0.0)])   # frames 8 .. 16 are zero


@pytest.mark.parametrize("space", ["mel_spectrogram", "wav_form"])
def test_gradient_is_exactly_zero_on_the_dead_span(space):
    from diffmusic_amd import inverse_problem as P
    from tests.test_gpu_operator_contract import _wave
    op = P.TimeFrequencyMaskOperator(16000, _dead_grid())
    span = op.dead_span(LEN)
    assert span == (2048, 256 * 14)
    wav, clean = _wave(1, LEN + 32, 0.05), _wave(2, LEN, 0.083)
    meas = op.forward(clean)
    assert float(meas[:, span[0]:span[1]].abs().max()) == 0.0
    loss, dwav = op.guidance(wav, LEN, meas, space)
    assert float(dwav[:, span[0]:span[1]].abs().max()) == 0.0 and float(dwav[:, :span[0]].abs().max()) > 0
    wav2 = wav.clone()
    wav2[:, span[0]:span[1]] = 7.0                                 # A does not see those samples
    loss2, dwav2 = op.guidance(wav2, LEN, meas, space)
    assert torch.equal(loss, loss2) and torch.equal(dwav, dwav2)


def test_step_with_the_dead_span_equals_the_step_without(nets, monkeypatch):
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    voc, vae, _, _ = nets
    op = P.TimeFrequencyMaskOperator(16000, _dead_grid())
    g = torch.Generator().manual_seed(5)
    clean = 0.3 * torch.sin(torch.arange(LEN) * 0.05)[None] * torch.tensor([[1.0], [0.6]]) + 0.05 * torch.randn(2, LEN, generator=g)
    x, e = torch.randn(2, 8, H, LAT_W, generator=g).cuda(), torch.randn(2, 8, H, LAT_W, generator=g).cuda()
    y = op.forward(clean.cuda())
    seen = []
    real = voc.forward

    def spy(mel, dead=None):
        seen.append(dead)
        return real(mel) if dead is None else real(mel, dead=dead)
    monkeypatch.setattr(voc, "forward", spy)

    def step():
        sched = get_scheduler("dps")(operator=op, **SCHED)
        sched.set_timesteps(200)
        return sched.step(e, 501, x, measurement=y, vae=vae, vocoder=voc, eta=0.0, ip_guidance_rate=5e-4, original_waveform_length=LEN,
                          supervised_space="mel_spectrogram")
    with_span = step()
    monkeypatch.setattr(op, "dead_span", lambda length: None)
    without = step()
    assert seen == [(2048, 3584), None]
    assert torch.equal(with_span.prev_sample, without.prev_sample) and torch.equal(with_span.loss, without.loss)


# ---- call level -----------------------------------------------------------------------------------------------------------------------
N_CALL, SECONDS = 4, 0.4


def test_call_equals_the_hand_written_loop():
    """`pipe(...)` of N = 4 steps with the operator against `_unet_eps` + `scheduler.step` written out: bit for bit, latents and losses."""
    from diffmusic_amd import inverse_problem as P
    from tests.test_gpu_declip import _pipe, _gens
    B = 2
    g = torch.Generator().manual_seed(11)
    pe = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    clean = 0.3 * torch.sin(torch.arange(LEN) * 0.05)[None] * torch.linspace(1.0, 0.6, B)[:, None] + 0.05 * torch.randn(B, LEN, generator=g)
    op = P.TimeFrequencyMaskOperator(16000, _dead_grid(), noiser=P.GaussianNoise(0.0))
    pipe = _pipe(op)
    y = op.forward(clean.cuda())
    got = pipe(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0,
               generator=_gens(B), output_type="latent").audios
    assert len(pipe.last_losses) == N_CALL and pipe.nan_restarts == 0
    got_losses = [l.reshape(-1).clone() for l in pipe.last_losses]
    dev = torch.device("cuda")
    s = pipe.scheduler
    gens = _gens(B)
    s.set_timesteps(N_CALL, device="cuda")
    x = pipe.prepare_latents(B, 8, 40, torch.float32, dev, gens, None)
    cond = pipe._prepare_cond(pe, None, 1, True, dev)
    losses = []
    for t in list(s._timesteps_host):
        eps = pipe._unet_eps(x, t, cond, pipe.default_guidance_scale, True)
        o = s.step(eps, t, x, eta=0.0, generator=gens, measurement=y, vae=pipe.vae, vocoder=pipe.vocoder, original_waveform_length=LEN,
                   ip_guidance_rate=5e-4, supervised_space="mel_spectrogram")
        x = o.prev_sample
        losses.append(o.loss)
    assert torch.equal(got, x)
    assert all(torch.equal(a, b.reshape(-1)) for a, b in zip(got_losses, losses))
    assert all(bool(torch.isfinite(l).all()) and bool((l > 0).all()) for l in got_losses)
