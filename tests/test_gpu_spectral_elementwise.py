"""-m gpu: every output element of the spectral front end (csrc/stft_mel.hip fused, csrc/mel.hip dense, chosen by csrc/audio_api.hip)
against the float64 model of tests/spectral_cases.py, inside the element-wise bound built from the number formats alone; exact zeros
where the contract says zero; every output buffer pre-filled with NaN and the sentinel intact wherever nothing may be written.

Each case runs through the public SpectralFrontend methods, the caller-owned / strided forms (`out=`, `dwav=`) included; for the
guidance pair with a caller-owned mel and a strided gradient, the two C entry points the public method itself calls.  The largest
error / bound ratio per route and output kind is carried in every assertion message and printed by the last test (`-s`)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import spectral_cases as S

pytestmark = pytest.mark.gpu

_WORST = {}
_FE = {}


def _frontend(c):
    from diffmusic_amd.inverse_problem.operator import SpectralFrontend
    key = (c.n_fft, c.hop, c.hann, c.bank)
    if key not in _FE:
        _FE[key] = SpectralFrontend(16000, c.n_fft, c.hop, 64, "hann" if c.hann else "rect", fb=S.bank(c.bank, c.n_fft // 2 + 1))
    return _FE[key]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _wav(c, i):
    """the case's waveform as a view into its storage: row stride and storage offset as the case says"""
    store = _dev(i.store)
    w = torch.as_strided(store, (c.B, c.Lfull), (c.stride, 1), c.offset)
    assert w.data_ptr() == store.data_ptr() + 4 * c.offset
    return w


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _check(c, route, kind, got, want, bnd):
    r = S.ratio(got.detach().cpu().numpy() if torch.is_tensor(got) else got, want, bnd)
    key = (route, kind)
    _WORST[key] = max(_WORST.get(key, 0.0), r)
    assert r <= 1.0, f"{c.name} {route} {kind}: error / bound = {r:.3g}; so far {_report()}"


def _report():
    return "  ".join(f"{k[0]}/{k[1]} {v:.3g}" for k, v in sorted(_WORST.items()))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guidance_raw(fe, c, wav, mask, ref, mel, loss, dwav, z, zmag, thr, L=None, power2=None, z_stride=None):
    """dmx_audio_guidance_{fwd,bwd}_shaped with caller-owned mel / loss / strided dwav -> (rc_fwd, rc_bwd)"""
    from diffmusic_amd import _lib
    lib = _lib.lib()
    L = c.L if L is None else L
    power2 = c.power2 if power2 is None else power2
    st = fe._get_state(c.B, max(L, c.L), wav.device)
    rs = 0 if (ref.shape[0] == 1 and c.B > 1) else ref[0].numel()
    ns = (z.stride(0) if z is not None else 0) if z_stride is None else z_stride
    a = fe._h.value
    rc1 = lib.dmx_audio_guidance_fwd_shaped(a, _p(wav), wav.stride(0), _p(mask), _p(ref), rs, _p(mel), _p(st), c.B, L, int(power2), int(c.to_db),
                                            c.lo, c.hi, _p(z), ns, _p(zmag), c.sigma, _p(thr), _stream())
    rc2 = lib.dmx_audio_guidance_bwd_shaped(a, _p(wav), wav.stride(0), _p(mask), _p(ref), rs, c.gscale, _p(loss), _p(dwav), dwav.stride(0),
                                            c.Lfull, _p(st), c.B, L, int(power2), int(c.to_db), c.lo, c.hi, _p(z), ns, _p(zmag), c.sigma,
                                            _p(thr), _stream())
    torch.cuda.synchronize()
    return rc1, rc2


def _all_nan(t):
    return bool(torch.isnan(t).all())


@pytest.mark.parametrize("c", [c for c in S.CASES if c.route == "fused" and not c.cot], ids=lambda c: c.name)
def test_fused_guidance_elementwise(c):
    i = S.inputs(c)
    fe = _frontend(c)
    assert fe.fused(c.L) and not S.refuses_guidance(c.n_fft, c.L, c.power2, i.zmag is not None, None if i.z is None else i.z.shape[1])
    r = S.model(c, i)
    q = S.bound(c, i, r, route="fused")
    wav, mask, ref, z, zmag, thr = _wav(c, i), _dev(i.mask), _dev(i.ref), _dev(i.z), _dev(i.zmag), _dev(i.thr)
    mel, loss, buf = _nan(c.B, i.T, 64), _nan(c.B), _nan(c.B, c.out_stride)
    rc = _guidance_raw(fe, c, wav, mask, ref, mel, loss, buf[:, :c.Lfull], z, zmag, thr)
    assert rc == (0, 0), rc
    _check(c, "fused", "mel", mel, r.o, q.o)
    _check(c, "fused", "loss", loss, r.loss, q.loss)
    _check(c, "fused", "dwav", buf[:, :c.L], r.dwav, q.dwav)
    g = buf.cpu().numpy()
    assert np.all(g[:, c.L:c.Lfull] == 0.0), "no gradient past the clip"
    assert np.all(np.isnan(g[:, c.Lfull:])), "row padding of the gradient was written"
    if i.mask is not None:
        assert np.all(g[:, :c.L][:, i.mask == 0] == 0.0), "masked samples carry a gradient"
    assert np.all(g[:, :c.L][:, r.count == 0] == 0.0), "samples no frame covers carry a gradient"
    # the public method: the same two launches, its own allocations -- bit for bit the same numbers
    loss2, dwav2 = fe.guidance(wav, c.L, ref, mask, c.power2, c.to_db, c.lo, c.hi, gscale=c.gscale, noise=z, noise_mag=zmag, sigma=c.sigma, thr=thr)
    assert dwav2.shape == (c.B, c.Lfull) and torch.equal(loss2, loss) and torch.equal(dwav2, buf[:, :c.Lfull])


def _transform_case(c, i, fe, wav, route):
    r = S.model(c, i)
    q = S.bound(c, i, r, route=route)
    mel = _nan(c.B, i.T, 64)
    out = fe.transform_fwd(wav, c.L, c.power2, c.to_db, c.lo, c.hi, out=mel)
    assert out.data_ptr() == mel.data_ptr()
    _check(c, route, "mel", mel, r.o, q.o)
    buf = _nan(c.B, c.out_stride + 3)
    fe.transform_bwd(_dev(i.dmel), dwav=buf[:, :c.L])
    torch.cuda.synchronize()
    _check(c, route, "dwav", buf[:, :c.L], r.dwav, q.dwav)
    g = buf.cpu().numpy()
    assert np.all(np.isnan(g[:, c.L:])), "transform_bwd wrote past L of a caller-owned gradient"
    assert np.all(g[:, :c.L][:, r.count == 0] == 0.0), "samples no frame covers carry a gradient"


@pytest.mark.parametrize("c", [c for c in S.CASES if c.route == "fused" and c.cot], ids=lambda c: c.name)
def test_fused_transform_vjp_elementwise(c):
    i = S.inputs(c)
    fe = _frontend(c)
    assert fe.fused(c.L)
    _transform_case(c, i, fe, _wav(c, i), "fused")


@pytest.mark.parametrize("c", [c for c in S.CASES if c.route == "dense"], ids=lambda c: c.name)
def test_dense_route_elementwise(c):
    """mel forward / backward (dense below the fused limit; at L = 2048 the fused kernels take it, and the dense chain is the
    stft_mag -> melscale -> stft_mag_bwd part: each against the model, never against each other)"""
    i = S.inputs(c)
    fe = _frontend(c)
    wav = _wav(c, i)
    assert not S.refuses_transform(c.n_fft, c.L)
    route = "fused" if fe.fused(c.L) else "dense"
    assert route == ("fused" if S.fused_route(c.n_fft, c.L) else "dense")
    _transform_case(c, i, fe, wav, route)
    # |STFT| and its backward: always the dense DFT
    rm = S.model(c, i, dmag=i.dmag)
    qm = S.bound(c, i, rm, route="dense", dmag=True)
    mag = fe.stft_mag(wav, c.L)
    assert mag.shape == (c.B, i.bins, i.T)
    _check(c, "dense", "mag", mag, rm.absX.transpose(0, 2, 1), qm.mag.transpose(0, 2, 1))
    buf = _nan(c.B, c.L + 5)
    fe.stft_mag_bwd(_dev(i.dmag), c.L, buf[:, :c.L])
    torch.cuda.synchronize()
    _check(c, "dense", "dmag", buf[:, :c.L], rm.dwav, qm.dwav)
    assert np.all(np.isnan(buf.cpu().numpy()[:, c.L:])), "stft_mag_bwd wrote past L"
    # MelScale on the magnitudes the kernel just produced (verified above; no tolerance is taken from them)
    lo, hi = 0.5, 20.0                                       # inside the data's range: both limits are met
    mel = fe.melscale(mag, lo, hi)
    want, bnd = S.melscale_model(mag.cpu().numpy(), i.fb, lo, hi)
    _check(c, "dense", "melscale", mel, want, bnd)


@pytest.mark.parametrize("n", [8 * 8192 - 1, 8 * 8192, 8 * 8192 + 77])
def test_l2norm_both_sides_of_its_switch(n):
    """dmx_l2_loss: one workgroup per clip below 8 * 8192 elements, chunked partial sums from there on; float64 sum as the model.
    Bound: the squared differences are summed at most 96 roundings deep on either path (64 per thread and a tree; 32 per thread, a
    tree, the chunk sums), so loss (1 +- gamma(98) + 2 u) and the gradient three more roundings."""
    from diffmusic_amd.inverse_problem.operator import l2_loss
    rng = np.random.default_rng(n)
    ref, pred = rng.standard_normal((1, n)).astype(np.float32), rng.standard_normal((3, n)).astype(np.float32)
    loss, g = l2_loss(_dev(ref), _dev(pred), gscale=0.5)
    d = ref.astype(np.float64) - pred.astype(np.float64)
    want = np.sqrt((d ** 2).sum(1))
    bl = want * (S.gamma(98) + 2 * S.U)
    wg = -d * (0.5 / want)[:, None]
    c = S.SimpleNamespace(name=f"l2norm_{n}")
    _check(c, "l2norm", "loss", loss, want, bl)
    _check(c, "l2norm", "grad", g, wg, np.abs(wg) * (3 * S.U + 1.01 * (bl / want)[:, None]))


def test_refusals_return_an_error_and_write_nothing():
    c = S.CASE["f2048_h160_mag"]
    i = S.inputs(c)
    fe = _frontend(c)
    wav, ref = _wav(c, i), _dev(i.ref)
    z = _dev(np.zeros((c.B, c.L), np.float32))
    zmag = _dev(np.zeros((c.B, i.bins, i.T), np.float32))

    def refused(**kw):
        mel, loss, buf = _nan(c.B, i.T, 64), _nan(c.B), _nan(c.B, c.Lfull)
        rc = _guidance_raw(fe, c, wav, None, ref, mel, loss, buf, kw.pop("z", None), kw.pop("zmag", None), None, **kw)
        return rc[0] != 0 and rc[1] != 0 and _all_nan(mel) and _all_nan(loss) and _all_nan(buf)

    assert S.refuses_guidance(1024, 2047, False, False, None) and refused(L=2047)                      # fused needs L >= 2048
    assert S.refuses_guidance(1024, 2048, True, True, None) and refused(zmag=zmag, power2=True)        # addmag only with magnitude
    assert S.refuses_guidance(1024, 2048, False, False, 2047) and refused(z=z, z_stride=2047)          # noise stride >= L
    rc = _guidance_raw(fe, c, wav, None, ref, _nan(c.B, i.T, 64), _nan(c.B), _nan(c.B, c.Lfull), None, None, None)
    assert rc == (0, 0)                                      # the same call without the offending argument is accepted
    # reflect padding needs L >= n_fft / 2 + 1
    from diffmusic_amd import _lib
    assert S.refuses_transform(1024, 512)
    mel = _nan(c.B, 1 + 512 // c.hop, 64)
    st = fe._get_state(c.B, c.L, wav.device)
    rc = _lib.lib().dmx_audio_transform_fwd(fe._h.value, _p(wav), wav.stride(0), _p(mel), _p(st), c.B, 512, 0, 0, c.lo, c.hi, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and _all_nan(mel)


def test_report_largest_ratios():
    """runs last (file order): the largest GPU error / bound per route and output kind of this session"""
    print("\nlargest error / bound: " + _report())
    assert all(v <= 1.0 for v in _WORST.values()), _report()
