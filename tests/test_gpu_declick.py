"""-m gpu: declicking -- the click detector, the per-clip masks and the output blend (csrc/declick.hip) stage by stage against
tests/declick_cases.py, through both bindings, and the DeclickOperator through guidance, schedulers, pipeline, track, mixture and lanes.

The reference has no declicking operator, so the oracle side is test-local: `_oracle_declick` subclasses the oracle's BaseOperator with
forward = mask * noiser(x) and transform = clamp(Wav2Mel, -80, 80), with the KERNEL's mask handed to it; the oracle schedulers take it as it
is and are given mask * y as their measurement."""
import ctypes as C
import json
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from tests import declick_cases as D                                                     # noqa: E402
from tests.test_gpu_step import HIFI, VAE, SCHED, H, W as LAT_W, LEN                     # noqa: E402

CANARY = 12345.678
_REPORT = {}


def _bindings():
    from diffmusic_amd import ops
    return (("torch_ops", ops.load()), ("ctypes", ops.ctypes_hip))


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _strided(a, off, pad=8):
    """numpy (B, n) -> a GPU view with row stride n + pad whose rows start `off` floats into their slots, canaries around them"""
    B, n = a.shape
    buf = torch.full((B, n + pad), CANARY, dtype=torch.float32, device="cuda")
    view = buf[:, off:off + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return view


def _detect(binding, y, c):
    a, e, sigma, flags, r = binding.click_detect(y, c.L, c.K, c.floor)
    mask, masked = binding.click_mask(flags, c.guard)
    return [a, e, sigma, flags, r, mask, masked]


def _row(outs, b):
    a, e, sigma, flags, r, mask, masked = [t[b].cpu().numpy() for t in outs]
    return SimpleNamespace(a=a, e=e, sigma=sigma, flags=flags, r=r, mask=mask, masked=int(masked))


def _fillers(L):
    rng = np.random.default_rng(77 + L)
    return (0.1 * rng.standard_normal((2, L))).astype(np.float32)


@pytest.fixture(scope="module")
def runs():
    """every case through both bindings: in a strided batch of three (row 1), alone, and as row 0 of a contiguous pair"""
    out = {}
    for c in D.CASES:
        y = c.make()
        fill = _fillers(c.L)
        batch = _strided(np.stack([fill[0], y, fill[1]]), 3)
        assert batch.stride(0) == c.L + 8 and batch.storage_offset() == 3
        alone = torch.from_numpy(y[None]).cuda()
        pair = torch.from_numpy(np.stack([y, fill[0]])).cuda()
        for name, binding in _bindings():
            out[c.name, name] = SimpleNamespace(y=y, batch=_detect(binding, batch, c), alone=_detect(binding, alone, c),
                                                pair=_detect(binding, pair, c), fill_alone=_detect(binding, torch.from_numpy(fill[:1]).cuda(), c))
    torch.cuda.synchronize()
    return out


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binding", ["torch_ops", "ctypes"])
@pytest.mark.parametrize("c", D.CASES, ids=lambda c: c.name)
def test_every_stage_lies_within_its_bound_or_is_exact(runs, c, binding):
    """Teacher-forced (tests/declick_cases.py): r against float64 within the format bound, a against float64 Levinson-Durbin on the kernel's
    own r within 8 times the emulation's own error, e against the float64 filter with the kernel's a, and sigma, flags, mask and masked bit
    for bit from the kernel's own e, sigma and flags."""
    run = runs[c.name, binding]
    out = _row(run.batch, 1)
    res = D.check_stages(c, run.y, out)
    _REPORT[c.name, binding] = dict(res, a_err_kernel=D.a_error(out), a_err_emulation=D.a_tolerance(c) / D.A_FACTOR)
    print(f"\n  {c.name}/{binding}: " + "  ".join(f"{k} {v:.3g}" for k, v in res.items()) +
          f"  |a32 - a64| kernel {D.a_error(out):.3e} emulation {D.a_tolerance(c) / D.A_FACTOR:.3e}")
    assert all(v <= 1.0 for v in res.values()), res


@pytest.mark.parametrize("c", D.CASES, ids=lambda c: c.name)
def test_the_mask_equals_the_float64_models_end_to_end(runs, c):
    """The kernel's mask may differ from the float64 model's only within `guard` of an undecided sample (model ratio within 1e-3 of 1);
    at most 1 % of a case's samples may be undecided."""
    run = runs[c.name, "torch_ops"]
    bad, undecided = D.end_to_end(c, run.y, _row(run.batch, 1).mask)
    print(f"\n  {c.name}: differing decided samples {bad}, undecided share {undecided:.5f}")
    assert undecided <= D.UNDECIDED_CAP, (c.name, undecided)
    assert bad == 0, (c.name, bad)


@pytest.mark.parametrize("c", D.CASES, ids=lambda c: c.name)
def test_a_clip_gives_the_same_bits_alone_in_a_batch_at_another_position_and_in_either_binding(runs, c):
    ref = runs[c.name, "torch_ops"]
    for binding in ("torch_ops", "ctypes"):
        run = runs[c.name, binding]
        for k in range(7):
            want = _bits(ref.alone[k][0])
            assert torch.equal(_bits(run.alone[k][0]), want), (c.name, binding, "alone", k)
            assert torch.equal(_bits(run.batch[k][1]), want), (c.name, binding, "batch row 1", k)
            assert torch.equal(_bits(run.pair[k][0]), want), (c.name, binding, "pair row 0", k)


@pytest.mark.parametrize("name", ["nan", "inf"])
def test_a_non_finite_sample_stays_in_its_frames_and_its_clip(runs, name):
    run = runs[name, "torch_ops"]
    out = _row(run.batch, 1)
    n = np.arange(D.BY_NAME[name].L)
    assert not out.a[1].any() and not out.a[2].any() and out.a[0].any() and out.a[3].any() and out.a[4].any()
    assert np.isfinite(out.e[(n < 2000) | (n > 2016)]).all() and not np.isfinite(out.e[2000:2017]).any()
    assert not out.flags[2001:2017].any() and out.flags[2000] == (0 if name == "nan" else 1)
    assert np.isfinite(out.sigma).all() and out.masked > 0
    for k in range(7):                                             # the neighbour in the batch keeps the bits it has alone
        assert torch.equal(_bits(run.batch[k][0]), _bits(run.fill_alone[k][0])), k
        assert torch.equal(_bits(run.pair[k][1]), _bits(run.fill_alone[k][0])), k


def _some_mask(L, B, seed):
    rng = np.random.default_rng(seed)
    m = np.ones((B, L), np.float32)
    for b in range(B):
        for p in rng.integers(0, L, size=max(1, L // 200)):
            m[b, p:p + int(rng.integers(1, 9))] = 0.0
    m[0, 0], m[B - 1, L - 1] = 0.0, 0.0
    return m


@pytest.mark.parametrize("L", [1, 17, 1025, 4133])
def test_mask_rows_and_blend_are_bit_exact(L):
    B, full = 3, L + 11
    rng = np.random.default_rng(L)
    xh, yh, mh = rng.standard_normal((B, full)).astype(np.float32), rng.standard_normal((B, full)).astype(np.float32), _some_mask(L, B, L)
    xh[1, L // 2] = np.nan
    x, y = _strided(xh, 1), _strided(yh, 2)
    for m_host, m_dev in ((mh, torch.from_numpy(mh).cuda()), (mh[1], torch.from_numpy(mh[1].copy()).cuda())):
        for name, binding in _bindings():
            for Ly in (L, full):
                got = binding.mask_rows(x, m_dev, L, Ly).cpu().numpy()
                want = D.ref_mask_rows(xh, m_host, L, Ly)
                assert got.shape == (B, Ly) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, Ly, m_host.ndim)
            for fade in (0, 1, 16, 64):
                got = binding.declick_blend(x, y, m_dev, L, fade).cpu().numpy()
                want = D.ref_blend(xh, yh, m_host, L, fade)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, fade, m_host.ndim)
    ones = torch.ones(L, device="cuda")
    assert torch.equal(_bits(_bindings()[0][1].declick_blend(x, y, ones, L, 16)), _bits(y[:, :L]))      # untouched samples: y's bits


def test_refusals_write_nothing():
    from diffmusic_amd import _lib
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L, full, B = 1500, 1510, 2
    F = D.frames(L)
    y = torch.randn(B, full, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def canaries():
        f = lambda *s: torch.full(s, CANARY, dtype=torch.float32, device="cuda")
        return dict(a=f(B, F, 16), e=f(B, L), sigma=f(B, F), flags=torch.full((B, L), 77, dtype=torch.uint8, device="cuda"), r=f(B, F, 17),
                    mask=f(B, L), masked=torch.full((B,), 77, dtype=torch.int32, device="cuda"), out=f(B, full))

    def untouched(o):
        torch.cuda.synchronize()
        return all(bool((t == (77 if t.dtype != torch.float32 else CANARY)).all()) for t in o.values())

    def detect(o, batch=B, L_=L, ys=full, K=5.0, floor=1e-5, null=None):
        ptr = {k: (C.c_void_p(0) if k == null else p(o[k])) for k in ("a", "e", "sigma", "flags", "r")}
        return lib.dmx_click_detect(C.c_void_p(0) if null == "y" else p(y), ys, ptr["a"], ptr["e"], ptr["sigma"], ptr["flags"], ptr["r"], batch, L_,
                                    K, floor, st)
    o = canaries()
    assert detect(o) == 0 and detect(o, null="r") == 0              # the same call with nothing wrong runs; r is optional
    torch.cuda.synchronize()
    assert not bool((o["e"] == CANARY).any())
    for what, word, kw in [("K 0", "threshold", dict(K=0.0)), ("K < 0", "threshold", dict(K=-1.0)), ("K nan", "threshold", dict(K=math.nan)),
                           ("K inf", "threshold", dict(K=math.inf)), ("floor < 0", "sigma_floor", dict(floor=-1e-9)),
                           ("floor nan", "sigma_floor", dict(floor=math.nan)), ("null y", "click_detect", dict(null="y")),
                           ("null e", "click_detect", dict(null="e")), ("batch 0", "click_detect", dict(batch=0)),
                           ("batch 65536", "click_detect", dict(batch=65536)), ("L 0", "click_detect", dict(L_=0)),
                           ("short stride", "click_detect", dict(ys=L - 1))]:
        o = canaries()
        assert detect(o, **kw) != 0 and untouched(o), what
        assert word in lib.dmx_last_error().decode(), (what, lib.dmx_last_error())
    flags = torch.zeros(B, L, dtype=torch.uint8, device="cuda")
    m = torch.ones(B, L, device="cuda")
    for what, word, call in [
            ("guard -1", "guard", lambda o: lib.dmx_click_mask(p(flags), p(o["mask"]), p(o["masked"]), B, L, -1, st)),
            ("guard 65", "guard", lambda o: lib.dmx_click_mask(p(flags), p(o["mask"]), p(o["masked"]), B, L, 65, st)),
            ("mask batch 0", "click_mask", lambda o: lib.dmx_click_mask(p(flags), p(o["mask"]), p(o["masked"]), 0, L, 3, st)),
            ("rows Ly < L", "mask_rows", lambda o: lib.dmx_mask_rows(p(y), full, p(m), L, p(o["out"]), B, L, L - 1, st)),
            ("rows mask stride", "mask_rows", lambda o: lib.dmx_mask_rows(p(y), full, p(m), L - 1, p(o["out"]), B, L, L, st)),
            ("rows x stride", "mask_rows", lambda o: lib.dmx_mask_rows(p(y), L - 1, p(m), L, p(o["out"]), B, L, L, st)),
            ("fade -1", "fade", lambda o: lib.dmx_declick_blend(p(y), full, p(y), full, p(m), L, p(o["out"]), B, L, -1, st)),
            ("fade 65", "fade", lambda o: lib.dmx_declick_blend(p(y), full, p(y), full, p(m), L, p(o["out"]), B, L, 65, st)),
            ("blend stride", "declick_blend", lambda o: lib.dmx_declick_blend(p(y), full, p(y), L - 1, p(m), L, p(o["out"]), B, L, 16, st))]:
        o = canaries()
        assert call(o) != 0 and untouched(o), what
        assert word in lib.dmx_last_error().decode(), (what, lib.dmx_last_error())
    for _, b in _bindings():                                        # and the bindings' own checks
        for bad in (lambda: b.click_detect(y, L, 0.0, 1e-5), lambda: b.click_detect(y, L, 5.0, -1.0), lambda: b.click_detect(y, full + 1, 5.0, 1e-5),
                    lambda: b.click_detect(y.cpu(), L, 5.0, 1e-5), lambda: b.click_mask(flags, 65), lambda: b.click_mask(flags, -1),
                    lambda: b.click_mask(flags.float(), 3), lambda: b.mask_rows(y, m, L, L - 1), lambda: b.mask_rows(y, m[:1].contiguous(), L, L),
                    lambda: b.mask_rows(y, m[:, :-1].contiguous(), L, L), lambda: b.mask_rows(y, m.cpu(), L, L),
                    lambda: b.declick_blend(y, y, m, L, 65), lambda: b.declick_blend(y, y[:1], m, L, 16)):
            with pytest.raises((RuntimeError, AssertionError)):
                bad()


def test_report_largest_ratios():
    if _REPORT:
        stages = ("r", "a", "e")
        worst = {s: max(_REPORT, key=lambda k: _REPORT[k][s]) for s in stages}
        print("\n  largest figure per bounded stage over %d runs: " % len(_REPORT) +
              "  ".join(f"{s} {_REPORT[worst[s]][s]:.4f} ({worst[s][0]})" for s in stages))
        print("  DECLICK_PARITY " + json.dumps({k[0]: dict(a_err_kernel=v["a_err_kernel"], a_err_emulation=v["a_err_emulation"], r=v["r"], e=v["e"])
                                                for k, v in _REPORT.items() if k[1] == "torch_ops"}))


# ---- operator level ---------------------------------------------------------------------------------------------------------------------
def _clips(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / 16000.0
    tones = torch.stack([0.3 * torch.sin(2 * np.pi * (220.0 * (b + 1)) * t) for b in range(B)])
    return (tones + 0.05 * torch.randn(B, n, generator=g)).cuda()


def _clicks(B, n, seed=0, rate=40.0):
    from diffmusic_amd.inverse_problem import dsp
    return dsp.click_train(n, 16000, rate, amplitude=(0.6, 0.9), max_width=3, seed=seed, batch=B).cuda()


def test_apply_and_adjoint():
    from diffmusic_amd import inverse_problem as P
    B, L, full = 3, 6400, 6437
    op = P.DeclickOperator()
    y = op.forward(_clips(B, L, 1), clicks=_clicks(B, L))
    m = op.detect(y)
    assert 0.0 < op.last_masked_fraction < 0.2 and m.shape == (B, L) and bool(((m == 0) | (m == 1)).all())
    assert abs(op.last_masked_fraction - float((m == 0).float().mean())) < 1e-9
    hit = _clicks(B, L) != 0
    assert float(((m == 0) & hit).sum()) >= 0.5 * float(hit.sum())       # most click samples are hidden
    x, w = torch.randn(B, full, device="cuda"), torch.randn(B, L, device="cuda")
    Ax, adjoint = op.apply(x, L, mask=m)
    assert torch.equal(Ax, x[:, :L] * m)
    Atw = adjoint(w, full)
    assert Atw.shape == (B, full) and float(Atw[:, L:].abs().max()) == 0.0
    lhs, rhs = (Ax.double() * w.double()).sum(), (x.double() * Atw.double()).sum()
    assert abs(float(lhs - rhs)) <= 1e-5 * abs(float(lhs))
    with pytest.raises(ValueError, match="mask= is needed"):
        op.apply(x, L)


@pytest.mark.parametrize("space", ["wav_form", "mel_spectrogram"])
@pytest.mark.parametrize("sigma", [0.0, 0.05])
def test_guidance_is_the_composition_of_its_parts(space, sigma, monkeypatch):
    from diffmusic_amd import inverse_problem as P, ops
    from diffmusic_amd.inverse_problem.operator import l2_loss
    L, pad, B = 6400, 32, 2
    op = P.DeclickOperator(noiser=P.GaussianNoise(sigma))
    wav = _clips(B, L + pad, 1)
    y = op.forward(_clips(B, L, 2), clicks=_clicks(B, L))
    z = torch.randn(B, L, device="cuda") if sigma > 0 else None
    loss, dwav = op.guidance(wav, L, y, space, noise=z)
    assert loss.shape == (B,) and dwav.shape == wav.shape and bool(torch.isfinite(dwav).all()) and float(loss.min()) > 0
    assert float(dwav[:, L:].abs().max()) == 0.0 and float(dwav.abs().max()) > 0
    m = P.DeclickOperator().detect(y)                          # the parts, written out: noise BEFORE the mask, both sides masked
    assert float((m == 0).sum()) > 0 and float(dwav[:, :L][m == 0].abs().max()) == 0.0
    h = ops.hip
    x = wav if z is None else h.noise_add(h.mask_mul(wav, None, L, L), z, sigma)
    pred, ym = h.mask_rows(x, m, L, L), h.mask_rows(y, m, L, L)
    if space == "wav_form":
        l2, dy = l2_loss(ym, pred)
    else:
        l2, dy = op.frontend.guidance(pred, L, op._mel(ym).clone(), lo=-80.0, hi=80.0)
    d2 = h.mask_rows(dy, m, L, L + pad)
    assert torch.equal(loss, l2) and torch.equal(dwav, d2)
    monkeypatch.setattr(ops, "USE_TORCH_OPS", False)               # the other binding: the same bits
    assert not ops.enabled()
    op.reset_cache()
    l3, d3 = op.guidance(wav, L, y, space, noise=z)
    monkeypatch.setattr(ops, "USE_TORCH_OPS", True)
    assert torch.equal(loss, l3) and torch.equal(dwav, d3)


def test_the_mask_is_cached_with_the_reference_and_pinned_masks_are_checked(monkeypatch):
    from diffmusic_amd import inverse_problem as P
    L, B = 6400, 2
    op = P.DeclickOperator()
    wav, y = _clips(B, L, 1), P.DeclickOperator().forward(_clips(B, L, 2), clicks=_clicks(B, L))
    calls = []
    inner = op.detect
    monkeypatch.setattr(op, "detect", lambda m: calls.append(1) or inner(m))
    first = op.guidance(wav, L, y, "mel_spectrogram")
    again = op.guidance(wav, L, y, "mel_spectrogram")
    assert len(calls) == 1 and torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    y.add_(0.0)                                                    # a new version of the measurement: detected again
    op.guidance(wav, L, y, "mel_spectrogram")
    assert len(calls) == 2
    op.cache_reference = False
    op.guidance(wav, L, y, "mel_spectrogram")
    op.guidance(wav, L, y, "mel_spectrogram")
    assert len(calls) == 4
    m = inner(y)
    pinned = P.DeclickOperator(mask=m.cpu())
    assert pinned.positional_state is not None
    got = pinned.guidance(wav, L, y, "wav_form")
    op.cache_reference = True
    want = op.guidance(wav, L, y, "wav_form")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    shared = P.DeclickOperator(mask=m[0].cpu())
    assert shared.positional_state is None and shared.guidance(wav, L, y, "wav_form")[0].shape == (B,)
    with pytest.raises(ValueError, match="holds a mask of shape"):
        pinned.guidance(wav[:1], L, y[:1], "wav_form")
    with pytest.raises(ValueError, match="holds a mask of shape"):
        shared.guidance(wav[:, :L - 1].contiguous(), L - 1, y[:, :L - 1].contiguous(), "wav_form")


def test_project_returns_the_measurements_bits_away_from_the_mask():
    from diffmusic_amd import inverse_problem as P
    L, B, fade = 6400, 2, 16
    op = P.DeclickOperator()
    y = op.forward(_clips(B, L, 2), clicks=_clicks(B, L))
    restored = _clips(B, L + 7, 3)
    op.guidance(restored, L, y, "wav_form")
    out = op.project(restored, y, fade=fade)
    m = op.detect(y)
    want = D.ref_blend(restored.cpu().numpy(), y.cpu().numpy(), m.cpu().numpy(), L, fade)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    far = torch.nn.functional.max_pool1d((m == 0).float()[:, None], 2 * fade + 1, 1, fade)[:, 0] == 0       # no zero within `fade`
    assert bool(far.any()) and torch.equal(_bits(out[far]), _bits(y[far])) and torch.equal(out[m == 0], restored[:, :L][m == 0])
    with pytest.raises(ValueError, match="fade"):
        op.project(restored, y, fade=65)


# ---- step level -----------------------------------------------------------------------------------------------------------------------
def _oracle_declick(sample_rate, mask, noiser=None):
    from oracle import audio, operators as O

    class OracleDeclick(O.BaseOperator):
        def __init__(self):
            self.wav2mel = audio.Wav2Mel(sample_rate)
            self.noiser = noiser

        def transform(self, a):
            return torch.clamp(self.wav2mel(a), min=-80, max=80)

        def forward(self, data, **k):                             # the step's noise BEFORE the mask
            return mask * (self.noiser(data) if self.noiser is not None else data)
    return OracleDeclick()


class _FixedNoiser:
    def __init__(self, sigma, z):
        self.sigma, self.z = sigma, z

    def __call__(self, data):
        return data + self.sigma * self.z


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


STEP_CASES = [("dps", 0.0, 5e-4, "mel_spectrogram", 501, True, 0.0), ("dps", 0.0, 5e-4, "wav_form", 996, True, 0.0),
              ("mpgd", 0.0, 5e-3, "mel_spectrogram", 251, True, 0.0), ("dsg", 1.0, 0.08, "mel_spectrogram", 501, False, 0.0),
              ("mpgd", 0.0, 5e-3, "wav_form", 251, True, 0.0), ("dsg", 1.0, 0.08, "wav_form", 501, False, 0.0),
              ("dps", 0.0, 5e-4, "mel_spectrogram", 501, True, 0.05)]


@pytest.mark.parametrize("name,eta,rate,space,t,per_clip,sigma", STEP_CASES,
                         ids=[f"{c[0]}-{c[3]}-{'clip' if c[5] else 'batch'}-sigma{c[6]}" for c in STEP_CASES])
def test_teacher_forced_declick_step(nets, name, eta, rate, space, t, per_clip, sigma):
    """The procedure and the bounds of tests/test_gpu_declip.py::test_teacher_forced_declipping_step: forward < 1e-4, loss < 1e-2, gradient
    cosine > 0.98, prev_sample < 1e-2, against torch autograd through the definition, the kernel's mask handed to the oracle-side operator."""
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
    z_meas = torch.randn(B, LEN, generator=g)
    z_step = torch.randn(B, LEN, generator=g)
    clicks = _clicks(B, LEN).cpu()
    op = P.DeclickOperator(16000, noiser=None)
    y_ref = clean + clicks + (sigma * z_meas if sigma > 0 else 0.0)
    rf = _rel(op.forward(clean.cuda(), clicks=clicks), clean + clicks)
    assert rf < 1e-4, "operator.forward"
    y = y_ref.cuda()
    mask = op.detect(y).cpu()                                  # the kernel's mask, handed to the oracle side
    share = float((mask == 0).float().mean())
    assert 0.0 < share < 0.3, share
    op.noiser = P.GaussianNoise(sigma)
    rop = _oracle_declick(16000, mask, _FixedNoiser(sigma, z_step) if sigma > 0 else None)
    rs = OS.get_scheduler(name)(operator=rop, per_clip_norm=per_clip, **SCHED)
    rs.set_timesteps(200)
    sched = get_scheduler(name)(operator=op, per_clip_norm=per_clip, **SCHED)
    sched.set_timesteps(200)
    sched.debug_keep_grad = True
    kw = dict(eta=eta, ip_guidance_rate=rate, original_waveform_length=LEN, supervised_space=space)
    noise_kw = dict(sample_noise=z.cuda()) if name == "dsg" else dict(variance_noise=None)
    opk = dict(noise=z_step.cuda()) if sigma > 0 else {}
    out = sched.step(e.cuda(), t, x.cuda(), measurement=y, vae=vae, vocoder=voc, op_kwargs=opk, **kw, **noise_kw)
    torch.cuda.synchronize()
    rnoise = dict(sample_noise=z) if name == "dsg" else dict(variance_noise=None)
    ro = rs.step(e, t, x, measurement=mask * y_ref, vae=rvae, vocoder=rvoc, **kw, **rnoise)
    rp = _rel(out.prev_sample, ro.prev_sample)
    rl = _rel(out.loss.reshape(-1), ro.loss.reshape(-1))
    rgr = _rel(sched.last_grad, ro.sample)
    cos = torch.nn.functional.cosine_similarity(sched.last_grad.cpu().flatten(), ro.sample.flatten(), dim=0).item()
    msg = (f"declick {name}/{space}/{'clip' if per_clip else 'batch'}/sigma={sigma}: forward {rf:.2e} prev {rp:.2e} loss {rl:.2e} grad {rgr:.2e} "
           f"cos {cos:.4f} masked {share:.4f}")
    print("\n  " + msg)
    assert _rel(out.pred_original_sample, ro.pred_original_sample) < 1e-4 or name == "mpgd"
    assert rl < 1e-2, msg
    assert cos > 0.98, msg
    assert rp < 1e-2, msg


# ---- call level -----------------------------------------------------------------------------------------------------------------------
SECONDS = 0.4


def _problem(B, T, seed=11):
    g = torch.Generator().manual_seed(seed)
    pe = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    return pe, _clips(B, T, seed)


def test_call_equals_the_hand_written_loop(monkeypatch):
    """`pipe(...)` with a DeclickOperator (auto-detection) against `_unet_eps` + `scheduler.step` written out: bit for bit, latents and
    losses; the ctypes binding gives the same bits; a (B, L) `mask=` is refused under lanes and shard by name."""
    from diffmusic_amd import inverse_problem as P, ops
    from tests.test_gpu_declip import _pipe, _gens, _hand_loop, N_CALL
    B = 3
    pe, clean = _problem(B, LEN)
    op = P.DeclickOperator(16000, noiser=P.GaussianNoise(0.0))
    pipe = _pipe(op)
    y = op.forward(clean, clicks=_clicks(B, LEN))
    call = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0)
    got = pipe(generator=_gens(B), output_type="latent", **call).audios
    assert len(pipe.last_losses) == N_CALL and pipe.nan_restarts == 0 and 0.0 < op.last_masked_fraction < 0.3
    got_losses = [l.reshape(-1).clone() for l in pipe.last_losses]
    x, losses = _hand_loop(pipe, pe, y, B)
    assert torch.equal(got, x)
    assert all(torch.equal(a, b.reshape(-1)) for a, b in zip(got_losses, losses))
    assert all(bool(torch.isfinite(l).all()) and bool((l > 0).all()) for l in got_losses)
    monkeypatch.setattr(ops, "USE_TORCH_OPS", False)
    assert not ops.enabled()
    got_ct = pipe(generator=_gens(B), output_type="latent", **call).audios
    monkeypatch.setattr(ops, "USE_TORCH_OPS", True)
    assert torch.equal(got, got_ct)
    pinned = _pipe(P.DeclickOperator(16000, mask=op.detect(y).cpu(), noiser=P.GaussianNoise(0.0)))
    assert torch.equal(pinned(generator=_gens(B), output_type="latent", **call).audios, got)        # the pinned mask: the same trajectory
    with pytest.raises(ValueError, match="DeclickOperator with a per-clip mask cannot run as clip lanes"):
        pinned(generator=_gens(B), output_type="latent", lanes=2, **call)
    with pytest.raises(ValueError, match="DeclickOperator with a per-clip mask cannot be sharded"):
        pinned(generator=_gens(B), output_type="latent", shard=True, **call)


def test_inside_a_track_equals_its_hand_loop():
    from diffmusic_amd import inverse_problem as P
    from tests.test_gpu_declip import _pipe, _gens, _hand_loop, N_CALL
    T, R = 16000, 1600                                       # windows of 6400 at 0, 4800, 9600
    lay = P.TrackLayout(T, LEN, R)
    assert lay.num_windows == 3
    pe, clean = _problem(3, T, seed=21)
    clean = clean[:1].contiguous()
    inner = P.DeclickOperator(16000, noiser=P.GaussianNoise(0.0))
    top = P.TrackOperator(inner, lay)
    pipe = _pipe(top, per_clip=False)
    y = top.forward(clean, clicks=_clicks(1, T))
    assert y.shape == (1, T)
    call = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0)
    lat = pipe(generator=_gens(3), output_type="latent", **call).audios
    assert lat.shape == (3, 8, 10, 16) and len(pipe.last_losses) == N_CALL and all(l.numel() == 1 for l in pipe.last_losses)
    assert 0.0 < inner.last_masked_fraction < 0.3                  # detection ran on the (1, T) track
    call_losses = [l.reshape(-1).clone() for l in pipe.last_losses]
    x, losses = _hand_loop(pipe, pe, y, 3)
    assert torch.equal(lat, x)
    assert all(torch.equal(a, b.reshape(-1)) for a, b in zip(call_losses, losses))
    assert all(bool(torch.isfinite(l).all()) and bool((l > 0).all()) for l in call_losses)


def test_inside_a_mixture_equals_its_hand_loop():
    from diffmusic_amd import inverse_problem as P
    from tests.test_gpu_mixture import _pipe, _gens, _hand_loop, N_CALL
    K = 2
    pe, clean = _problem(K, LEN, seed=31)
    inner = P.DeclickOperator(16000, noiser=P.GaussianNoise(0.0))
    top = P.MixtureOperator(inner, K, [1.0, 0.5])
    pipe = _pipe(top)
    y = top.forward(clean, clicks=_clicks(1, LEN))
    assert y.shape == (1, LEN)
    call = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0)
    lat = pipe(generator=_gens(K), output_type="latent", **call).audios
    assert len(pipe.last_losses) == N_CALL and all(l.numel() == 1 for l in pipe.last_losses)
    got_losses = list(pipe.last_losses)
    _, x, losses = _hand_loop(pipe, pe, y, K)
    assert torch.equal(lat, x)
    assert all(torch.equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(got_losses, losses))
    assert all(bool(torch.isfinite(l).all()) and bool((l > 0).all()) for l in got_losses)


def test_clip_lanes_with_auto_detection_equal_the_plain_loop():
    """lanes = 2 on four clips equals the two clip groups run with lanes = 1, bit for bit (the detected mask is a function of the
    measurement's rows: no per-position state), the procedure of tests/test_gpu_lanes.py on the small nets."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.pipelines.lanes import split_sizes
    from tests.test_gpu_pipeline import UNET, _build
    B, N = 4, 4
    op = P.DeclickOperator(16000, noiser=P.GaussianNoise(0.0))
    pipe = _build("musicldm", UNET, "dps", op)
    g = torch.Generator().manual_seed(3)
    pe = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    lat0 = torch.randn(B, 8, 10, 16, generator=g)
    y = op.forward(_clips(B, LEN, 3), clicks=_clicks(B, LEN))

    def call(ids, lanes):
        gens = [torch.Generator().manual_seed(100 + k) for k in ids]
        out = pipe(prompt_embeds=pe[ids], negative_prompt_embeds=ne[ids], audio_length_in_s=SECONDS, num_inference_steps=N, guidance_scale=2.0,
                   latents=lat0[ids].clone(), measurement=y[ids].contiguous(), ip_guidance_rate=5e-4, eta=0.0, generator=gens,
                   show_progress=False, output_type="latent", lanes=lanes)
        return out.audios, [l.reshape(-1).clone() for l in pipe.last_losses]
    got, losses = call(list(range(B)), 2)
    assert got.shape == (B, 8, 10, 16) and len(losses) == N
    o = 0
    for n in split_sizes(B, 2):
        ids = list(range(o, o + n))
        ref, ref_losses = call(ids, 1)
        assert torch.equal(got[ids], ref), f"lane {ids}: latents differ from the plain loop on those clips"
        assert all(torch.equal(losses[k][ids], ref_losses[k]) for k in range(N)), f"lane {ids}: a loss differs"
        o += n
