"""-m gpu: wow and flutter (csrc/warp.hip, inverse_problem/operator.py TimeWarpOperator).

Kernel level: every case of tests/warp_cases.py against the float64 model, EVERY element of y and dx within the bound derived from the
number formats, through both bindings (bit-identical); the exactness properties; a clip alone, in a batch and at another batch position
gives the same bits; the NaN rule; refusals; out-of-contract curves touch nothing outside their own outputs.  Operator level: `apply` /
`adjoint` with a shared curve and with per-clip curves.  Step level: teacher-forced steps against `oracle.schedulers` around an oracle
operator defined here -- torch autograd through the definition -- with the bounds of tests/test_gpu_declip.py.  Call level: `pipe(...)`
equals a hand-written loop bit for bit, alone, inside a TrackOperator and inside a MixtureOperator; clip lanes equal the plain loop."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import warp_cases as W                                                      # noqa: E402
from tests.test_warp_bound_host import torch_warp                                      # noqa: E402
from tests.test_gpu_step import HIFI, VAE, SCHED, H, W as LAT_W, LEN                   # noqa: E402

CANARY = 12345.678
_REPORT = {}


def _bindings():
    from diffmusic_amd import ops
    return (("torch_ops", ops.load()), ("ctypes", ops.ctypes_hip))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _strided(a, off, pad=8):
    """numpy (B, n) -> a GPU view with row stride n + pad whose rows start `off` floats into their slots, canaries around them"""
    B, n = a.shape
    buf = torch.full((B, n + pad), CANARY, dtype=torch.float32, device="cuda")
    view = buf[:, off:off + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return view


def _dev_case(c):
    i = W.inputs(c)
    x = _strided(i.store, c.off)
    assert x.stride(0) == c.stride + 8 and x.shape[1] >= c.L
    return i, x, torch.from_numpy(i.dy).cuda(), torch.from_numpy(i.delay).cuda()


def _run(binding, c, x, dy, delay):
    return binding.warp_fwd(x, delay, c.L), binding.warp_bwd(dy, delay, c.L, c.full)


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c.name)
def test_kernels_lie_within_the_bound_in_every_element(c):
    i, x, dy, delay = _dev_case(c)
    r, qy, rb, qdx = W.reference(c)
    outs = []
    for name, binding in _bindings():
        y, dx = _run(binding, c, x, dy, delay)
        assert y.shape == (c.B, c.L) and y.is_contiguous() and dx.shape == (c.B, c.full) and dx.is_contiguous()
        got = {"y": W.ratio(y.cpu().numpy(), r.y, qy), "dx": W.ratio(dx[:, :c.L].cpu().numpy(), rb.dx, qdx)}
        _REPORT[c.name] = max(_REPORT.get(c.name, 0.0), *got.values())
        print(f"\n  {c.name}/{name}: largest |kernel - model| / bound " + " ".join(f"{k} {v:.4f}" for k, v in got.items()))
        assert all(v <= 1.0 for v in got.values()), (c.name, name, got)
        assert bool((_bits(dx[:, c.L:]) == 0).all()), "dx[:, L:full] is +0.0f"
        outs.append((y, dx))
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b)), "the two bindings are bit-identical"
    if c.signal == "silence":
        assert bool((_bits(outs[0][0]) == 0).all())


def test_zero_delay_is_the_identity_and_an_integer_delay_a_shift_bit_for_bit():
    L, full = 5000, 5003
    K = W.knots(L)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, full, generator=g).cuda()
    dy = torch.randn(2, L, generator=g).cuda()
    for _, binding in _bindings():
        zero = torch.zeros(K, device="cuda")
        assert torch.equal(_bits(binding.warp_fwd(x, zero, L)), _bits(x[:, :L]))
        back = binding.warp_bwd(dy, zero, L, full)
        assert torch.equal(_bits(back[:, :L]), _bits(dy)) and bool((_bits(back[:, L:]) == 0).all())
        for s in (7, -130, 4096, -4096):
            d = torch.full((K,), float(s), device="cuda")
            want, tr = torch.zeros(2, L, device="cuda"), torch.zeros(2, full, device="cuda")
            if s > 0:
                want[:, :L - s] = x[:, s:L]
                tr[:, s:L] = dy[:, :L - s]                      # the transpose is the opposite shift
            else:
                want[:, -s:] = x[:, :L + s]
                tr[:, :L + s] = dy[:, -s:]
            assert torch.equal(_bits(binding.warp_fwd(x, d, L)), _bits(want)), s
            assert torch.equal(_bits(binding.warp_bwd(dy, d, L, full)), _bits(tr)), s


@pytest.mark.parametrize("name", ["L65", "L1000", "L6400_zigzag", "L20037_stride", "L70000", "L70000_shared"])
def test_a_clip_gives_the_same_bits_alone_in_a_batch_and_at_another_position(name):
    from diffmusic_amd import ops
    c = W.CASE[name]
    i, x, dy, delay = _dev_case(c)
    first = _run(ops.hip, c, x, dy, delay)
    again = _run(ops.hip, c, x, dy, delay)
    for a, b in zip(first, again):
        assert torch.equal(_bits(a), _bits(b)), "two runs are bit-equal"
    for b in range(c.B):
        alone = _run(ops.hip, c, x[b:b + 1], dy[b:b + 1], delay if c.shared else delay[b:b + 1].contiguous())
        for a, f in zip(alone, first):
            assert torch.equal(_bits(a[0]), _bits(f[b])), (name, b)
    xs, dys = x.flip(0).contiguous(), dy.flip(0).contiguous()     # contiguous rows at the mirrored position: another alignment too
    swapped = _run(ops.hip, c, xs, dys, delay if c.shared else delay.flip(0).contiguous())
    for a, f in zip(swapped, first):
        assert torch.equal(_bits(a.flip(0)), _bits(f)), "neither the batch position nor the load path matters"
    if c.shared:                                                  # one curve for every clip = that curve once per clip
        rows = _run(ops.hip, c, x, dy, delay[None].expand(c.B, -1).contiguous())
        for a, f in zip(rows, first):
            assert torch.equal(_bits(a), _bits(f))


@pytest.mark.parametrize("name", ["L1000_integers", "L6400_zigzag"])
def test_a_nan_reaches_exactly_the_outputs_whose_taps_include_it(name):
    """A NaN at x[m]: y[n] is NaN exactly for the n with i(n) - 1 <= m <= i(n) + 2 -- a zero weight does not shield it (the integer case
    has f = 0, weights 0, 1, 0, 0) -- and bit-equal to the clean run elsewhere.  A NaN at dy[n]: dx is NaN exactly on the taps of n inside
    the clip.  Other clips are untouched.  i(n) is taken from the fp32 emulation of the kernel's own arithmetic."""
    from diffmusic_amd import ops
    c = W.CASE[name]
    i, x, dy, delay = _dev_case(c)
    clean = _run(ops.hip, c, x, dy, delay)
    b, m, n0 = 1, 417, 530
    i32, _ = W.positions32(i.delay[b], c.L)
    hit = torch.from_numpy((i32 - 1 <= m) & (m <= i32 + 2)).cuda()
    assert 2 <= int(hit.sum()) <= 6
    taps = torch.zeros(c.full, dtype=torch.bool, device="cuda")
    for k in range(-1, 3):
        if 0 <= i32[n0] + k < c.L:
            taps[i32[n0] + k] = True
    assert int(taps.sum()) == 4
    xn, dyn = x.clone(), dy.clone()
    xn[b, m] = float("nan")
    dyn[b, n0] = float("nan")
    for _, binding in _bindings():
        y, dx = _run(binding, c, xn, dyn, delay)
        assert torch.equal(torch.isnan(y[b]), hit) and torch.equal(torch.isnan(dx[b]), taps)
        assert torch.equal(_bits(y[b])[~hit], _bits(clean[0][b])[~hit]) and torch.equal(_bits(dx[b])[~taps], _bits(clean[1][b])[~taps])
        for other in (0, 2):
            assert torch.equal(_bits(y[other]), _bits(clean[0][other])) and torch.equal(_bits(dx[other]), _bits(clean[1][other]))


def _raw_calls(L, full, B, xs):
    """the C entries on canary-filled outputs with canaries behind them -> fwd(...), bwd(...) returning (rc, y / dx, tail canaries intact)"""
    from diffmusic_amd import _lib
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pad = 64

    def fwd(x, delay, ds, batch=B, L_=L, xs_=xs, null=None):
        y = torch.full((B * L + pad,), CANARY, dtype=torch.float32, device="cuda")
        ptr = {"x": x.data_ptr(), "delay": delay.data_ptr(), "y": y.data_ptr()}
        if null:
            ptr[null] = 0
        rc = lib.dmx_warp_fwd(C.c_void_p(ptr["x"]), xs_, C.c_void_p(ptr["delay"]), ds, C.c_void_p(ptr["y"]), batch, L_, st)
        torch.cuda.synchronize()
        return rc, y[:B * L].view(B, L), bool((y[B * L:] == CANARY).all())

    def bwd(dy, delay, ds, batch=B, L_=L, full_=full, null=None):
        dx = torch.full((B * full + pad,), CANARY, dtype=torch.float32, device="cuda")
        ptr = {"dy": dy.data_ptr(), "delay": delay.data_ptr(), "dx": dx.data_ptr()}
        if null:
            ptr[null] = 0
        rc = lib.dmx_warp_bwd(C.c_void_p(ptr["dy"]), C.c_void_p(ptr["delay"]), ds, C.c_void_p(ptr["dx"]), batch, L_, full_, st)
        torch.cuda.synchronize()
        return rc, dx[:B * full].view(B, full), bool((dx[B * full:] == CANARY).all())
    return lib, fwd, bwd


def test_refusals_write_nothing():
    from diffmusic_amd import ops
    L, full, B = 1500, 1510, 2
    K = W.knots(L)
    x = torch.randn(B, full, device="cuda")
    dy = torch.randn(B, L, device="cuda")
    delay = torch.zeros(B, K + 3, device="cuda")
    lib, fwd, bwd = _raw_calls(L, full, B, full)
    for ds in (0, K, K + 3):                                      # the same calls with nothing wrong run
        rc, y, tail = fwd(x, delay, ds)
        assert rc == 0 and tail and torch.equal(y, x[:, :L])
        rc, dx, tail = bwd(dy, delay, ds)
        assert rc == 0 and tail and torch.equal(dx[:, :L], dy)
    for what, kw in [("null x", dict(null="x")), ("null delay", dict(null="delay")), ("null y", dict(null="y")), ("batch 0", dict(batch=0)),
                     ("batch 65536", dict(batch=65536)), ("L 0", dict(L_=0)), ("L above 2^30", dict(L_=(1 << 30) + 1, xs_=(1 << 30) + 1)),
                     ("short x stride", dict(xs_=L - 1)), ("delay stride below H + 1", dict(ds=K - 1)), ("delay stride 1", dict(ds=1)),
                     ("negative delay stride", dict(ds=-K))]:
        kw = dict(kw)
        rc, y, tail = fwd(x, delay, kw.pop("ds", K), **kw)
        assert rc != 0 and tail and bool((y == CANARY).all()) and lib.dmx_last_error(), ("warp_fwd", what)
    for what, kw in [("null dy", dict(null="dy")), ("null delay", dict(null="delay")), ("null dx", dict(null="dx")), ("batch 0", dict(batch=0)),
                     ("batch 65536", dict(batch=65536)), ("L 0", dict(L_=0)), ("full < L", dict(full_=L - 1)),
                     ("full above 2^30", dict(full_=(1 << 30) + 1)), ("delay stride below H + 1", dict(ds=K - 1)),
                     ("negative delay stride", dict(ds=-1))]:
        kw = dict(kw)
        rc, dx, tail = bwd(dy, delay, kw.pop("ds", K), **kw)
        assert rc != 0 and tail and bool((dx == CANARY).all()) and lib.dmx_last_error(), ("warp_bwd", what)
    good = torch.zeros(B, K, device="cuda")
    for _, binding in _bindings():                                # and the bindings' own checks
        for bad in (lambda: binding.warp_fwd(x, good, full + 1), lambda: binding.warp_fwd(x.cpu(), good, L), lambda: binding.warp_fwd(x, good.cpu(), L),
                    lambda: binding.warp_fwd(x, good[:, :-1].contiguous(), L), lambda: binding.warp_fwd(x, good[:1].contiguous(), L),
                    lambda: binding.warp_fwd(x, good.double(), L), lambda: binding.warp_fwd(x, delay[:, :K], L),
                    lambda: binding.warp_bwd(dy, good, L, L - 1), lambda: binding.warp_bwd(dy, good, L - 1, full),
                    lambda: binding.warp_bwd(dy, good[0, :-1].contiguous(), L, full), lambda: binding.warp_bwd(x[:, :L], good, L, full)):
            with pytest.raises((RuntimeError, AssertionError)):
                bad()
    assert ops.hip.warp_bwd(dy, good[0].contiguous(), L, full).shape == (B, full)


def test_out_of_contract_curves_stay_inside_their_buffers():
    """The C entries cannot see the knots' values, so the kernels are safe for any bits (read through in csrc/warp.hip: every index is
    compared with [0, L) before its load, both loops of the transpose have constant trip bounds, the float-to-int conversion follows a
    clamp).  NaN knots, +-inf, 1e30, a +-2000 zigzag, on canary-padded strided rows at L = 1500: the calls return, the canaries behind the
    outputs are intact, no canary around x was read into a finite output, a non-finite delta gives y = NaN, and the clip with a good curve in
    the same batch keeps its bits."""
    L, full, B = 1500, 1510, 5
    K = W.knots(L)
    rng = np.random.default_rng(9)
    x = _strided(rng.standard_normal((B, full)).astype(np.float32), 1)
    dy = torch.from_numpy(rng.standard_normal((B, L)).astype(np.float32)).cuda()
    j = np.arange(K)
    good = W.random_walk(rng, K, 4.0, 10.0)
    nan_some = good.copy()
    nan_some[5:9] = np.nan
    huge = np.where(j % 3 == 0, 1e30, np.where(j % 3 == 1, -1e30, 0.0)).astype(np.float32)
    infs = good.copy()
    infs[3], infs[11] = np.inf, -np.inf
    zig = np.where(j % 2 == 0, 2000.0, -2000.0).astype(np.float32)
    delay = torch.from_numpy(np.stack([nan_some, huge, good, infs, zig])).cuda()
    lib, fwd, bwd = _raw_calls(L, full, B, x.stride(0))
    rc, y, tail = fwd(x, delay, K)
    assert rc == 0 and tail
    rc, dx, tail2 = bwd(dy, delay, K)
    assert rc == 0 and tail2
    _, y_good, _ = _raw_calls(L, full, 1, x.stride(0))[1](x[2:3], delay[2:3].contiguous(), K, batch=1)
    _, dx_good, _ = _raw_calls(L, full, 1, x.stride(0))[2](dy[2:3].contiguous(), delay[2:3].contiguous(), K, batch=1)
    assert torch.equal(_bits(y[2]), _bits(y_good[0])) and torch.equal(_bits(dx[2]), _bits(dx_good[0]))
    assert bool(torch.isfinite(y[2]).all()) and bool(torch.isfinite(dx[2]).all())
    assert bool(torch.isnan(y[0, 64 * 4 + 1:64 * 9]).all()) and bool(torch.isfinite(y[0, :64 * 4]).all()) and bool(torch.isfinite(y[0, 64 * 9:]).all())
    assert bool(torch.isnan(y[3, 64 * 2 + 1:64 * 4]).all()) and bool(torch.isnan(y[3, 64 * 10 + 1:64 * 12]).all())
    ymax, gmax = float(x[:, :L].abs().max()), float(dy.abs().max())
    fin = torch.isfinite(y)
    assert float(y[fin].abs().max()) <= 2.0 * ymax                 # four taps, |w| sums to at most 1.25: no canary was read
    fin = torch.isfinite(dx[:, :L])
    assert float(dx[:, :L][fin].abs().max()) <= 8.0 * gmax         # at most 8 terms of weight at most 1
    assert bool((_bits(dx[:, L:]) == 0).all())


def test_report_largest_ratios():
    if _REPORT:
        worst = max(_REPORT, key=_REPORT.get)
        print(f"\n  largest |kernel - model| / bound over {len(_REPORT)} cases: {_REPORT[worst]:.4f} ({worst})")


# ---- operator level ---------------------------------------------------------------------------------------------------------------------
def _clips(B, n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / 16000.0
    tones = torch.stack([0.3 * torch.sin(2 * np.pi * (220.0 * (b + 1)) * t) for b in range(B)])
    return (tones + 0.05 * torch.randn(B, n, generator=g)).cuda()


def _curve(length, depth=1.0, seed=0):
    from diffmusic_amd import inverse_problem as P
    return P.wow_curve(length, 16000, ((2.0 + seed, 2.0 * depth, 30.0 * seed), (9.0, 0.5 * depth, 0.0)), speed_percent=0.5 * depth)


@pytest.mark.parametrize("per_clip", [False, True], ids=["shared", "per_clip"])
def test_apply_and_adjoint(per_clip):
    from diffmusic_amd import inverse_problem as P, ops
    length, pad, B = 6400, 32, 3
    curve = np.stack([_curve(length, seed=b) for b in range(B)]) if per_clip else _curve(length)
    op = P.TimeWarpOperator(16000, delay=curve)
    x = _clips(B, length + pad, 4)
    y, adjoint = op.apply(x, length)
    d = op.delay_on(x.device)
    assert d is op.delay_on(x.device) and tuple(d.shape) == tuple(curve.shape)
    assert torch.equal(y, ops.hip.warp_fwd(x, d, length)) and y.shape == (B, length)
    r = W.model(x.cpu().numpy(), curve, length)
    assert W.ratio(y.cpu().numpy(), r.y, W.bound(r)) <= 1.0
    assert float((y - x[:, :length]).abs().max()) > 0.05           # the curve acts
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).cuda()
    got = adjoint(w, length + pad)
    assert got.shape == x.shape and torch.equal(got, ops.hip.warp_bwd(w, d, length, length + pad)) and float(got[:, length:].abs().max()) == 0.0
    rb = W.model_bwd(w.cpu().numpy(), curve, length, r)
    assert W.ratio(got[:, :length].cpu().numpy(), rb.dx, W.bound_bwd(r, rb, w.cpu().numpy())) <= 1.0
    lhs, rhs = float((y.double() * w.double()).sum()), float((x.double() * got.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * float((y.double().abs() * w.double().abs()).sum()), (lhs, rhs)      # <A x, w> = <x, A^T w>
    assert torch.equal(adjoint(w[:, :].t().contiguous().t(), length + pad), got)                        # a strided cotangent is made contiguous
    assert torch.equal(op.forward(x[:, :length].contiguous()), ops.hip.warp_fwd(x[:, :length].contiguous(), d, length))
    fixed = torch.randn(B, length, generator=torch.Generator().manual_seed(4)).cuda()
    op.noiser = lambda v: v + 0.1 * fixed
    assert torch.equal(op.forward(x[:, :length].contiguous()), op.apply(x[:, :length].contiguous(), length)[0] + 0.1 * fixed)
    if per_clip:
        with pytest.raises(ValueError, match="3 per-clip"):
            op.apply(x[:2], length)
    else:
        assert torch.equal(op.apply(x[:2], length)[0], y[:2])


def test_a_wrong_length_is_refused_by_name():
    from diffmusic_amd import inverse_problem as P
    op = P.TimeWarpOperator(16000, delay=_curve(6400))
    x = _clips(2, 6500, 1)
    for call in (lambda: op.apply(x, 6500), lambda: op.forward(x), lambda: op.guidance(x, 6336, x[:, :6336].contiguous(), "mel_spectrogram")):
        with pytest.raises(ValueError, match=r"warp_knots\(\d+\) = \d+ knots"):
            call()
    assert op.apply(x, 6400)[0].shape == (2, 6400) and op.apply(x, 6337)[0].shape == (2, 6337)      # any length with the same number of knots


@pytest.mark.parametrize("space", ["wav_form", "mel_spectrogram"])
def test_guidance_is_the_composition_of_its_parts(space, monkeypatch):
    from diffmusic_amd import inverse_problem as P, ops
    from tests.test_gpu_operator_contract import _chain
    length, pad, B = 6400, 32, 2
    op = P.TimeWarpOperator(16000, delay=_curve(length), noiser=P.GaussianNoise(0.0))
    wav, clean = _clips(B, length + pad, 1), _clips(B, length, 2)
    meas = op.forward(clean)
    loss, dwav = op.guidance(wav, length, meas, space)
    assert loss.shape == (B,) and dwav.shape == wav.shape and bool(torch.isfinite(dwav).all()) and float(loss.min()) > 0
    assert float(dwav[:, length:].abs().max()) == 0.0 and float(dwav.abs().max()) > 0
    l2, d2 = _chain(op, wav, length, meas, space, None, {}, fused_pair_on_y=True)
    assert torch.equal(loss, l2) and torch.equal(dwav, d2)
    monkeypatch.setattr(ops, "USE_TORCH_OPS", False)               # the other binding: the same bits
    assert not ops.enabled()
    l3, d3 = op.guidance(wav, length, meas, space)
    monkeypatch.setattr(ops, "USE_TORCH_OPS", True)
    assert torch.equal(loss, l3) and torch.equal(dwav, d3)


# ---- step level -----------------------------------------------------------------------------------------------------------------------
def _oracle_warp(sample_rate, delay, noiser=None):
    from oracle import audio, operators as O

    class OracleWarp(O.BaseOperator):
        def __init__(self):
            self.wav2mel = audio.Wav2Mel(sample_rate)
            self.noiser = noiser

        def transform(self, a):
            return torch.clamp(self.wav2mel(a), min=-80, max=80)

        def forward(self, data, **k):
            y = torch_warp(data, delay)
            return self.noiser(y) if self.noiser is not None else y
    return OracleWarp()


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


STEP_CASES = [("dps", 0.0, 5e-4, "mel_spectrogram", 501, True, 0.0, False), ("dps", 0.0, 5e-4, "wav_form", 996, True, 0.0, True),
              ("mpgd", 0.0, 5e-3, "mel_spectrogram", 251, True, 0.0, False), ("dsg", 1.0, 0.08, "mel_spectrogram", 501, False, 0.0, True),
              ("dps", 0.0, 5e-4, "mel_spectrogram", 501, True, 0.05, False)]


@pytest.mark.parametrize("name,eta,rate,space,t,per_clip,sigma,curves", STEP_CASES,
                         ids=[f"{c[0]}-{c[3]}-{'clip' if c[5] else 'batch'}-sigma{c[6]}-{'curves' if c[7] else 'shared'}" for c in STEP_CASES])
def test_teacher_forced_time_warp_step(nets, name, eta, rate, space, t, per_clip, sigma, curves):
    """The procedure and the bounds of tests/test_gpu_declip.py::test_teacher_forced_declipping_step: forward < 1e-4, loss < 1e-2, gradient
    cosine > 0.98, prev_sample < 1e-2, against torch autograd through the definition."""
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
    curve = np.stack([_curve(LEN, seed=b) for b in range(B)]) if curves else _curve(LEN)
    op = P.TimeWarpOperator(16000, delay=curve, noiser=None)
    rop = _oracle_warp(16000, torch.from_numpy(curve))
    y_clean = rop.forward(clean)
    assert float((y_clean - clean).abs().max()) > 0.05             # the curve acts
    rf = _rel(op.forward(clean.cuda()), y_clean)
    print(f"\n  operator.forward rel-L2 {rf:.2e}")
    assert rf < 1e-4, "operator.forward"
    rop.noiser = _FixedNoiser(sigma, z_meas) if sigma > 0 else None
    y_ref = rop.forward(clean)
    y = y_ref.cuda()
    op.noiser = P.GaussianNoise(sigma)
    rs = OS.get_scheduler(name)(operator=rop, per_clip_norm=per_clip, **SCHED)
    rs.set_timesteps(200)
    sched = get_scheduler(name)(operator=op, per_clip_norm=per_clip, **SCHED)
    sched.set_timesteps(200)
    sched.debug_keep_grad = True
    rop.noiser = _FixedNoiser(sigma, z_step) if sigma > 0 else None
    kw = dict(eta=eta, ip_guidance_rate=rate, original_waveform_length=LEN, supervised_space=space)
    noise_kw = dict(sample_noise=z.cuda()) if name == "dsg" else dict(variance_noise=None)
    opk = dict(noise=z_step.cuda()) if sigma > 0 else {}
    out = sched.step(e.cuda(), t, x.cuda(), measurement=y, vae=vae, vocoder=voc, op_kwargs=opk, **kw, **noise_kw)
    torch.cuda.synchronize()
    rnoise = dict(sample_noise=z) if name == "dsg" else dict(variance_noise=None)
    ro = rs.step(e, t, x, measurement=y_ref, vae=rvae, vocoder=rvoc, **kw, **rnoise)
    rp = _rel(out.prev_sample, ro.prev_sample)
    rl = _rel(out.loss.reshape(-1), ro.loss.reshape(-1))
    rgr = _rel(sched.last_grad, ro.sample)
    cos = torch.nn.functional.cosine_similarity(sched.last_grad.cpu().flatten(), ro.sample.flatten(), dim=0).item()
    msg = (f"time warp {name}/{space}/{'clip' if per_clip else 'batch'}/sigma={sigma}/{'curves' if curves else 'shared'}: prev {rp:.2e} "
           f"loss {rl:.2e} grad {rgr:.2e} cos {cos:.4f}")
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
    """`pipe(...)` with a TimeWarpOperator (per-clip curves) against `_unet_eps` + `scheduler.step` written out: bit for bit, latents and
    losses; the ctypes binding gives the same bits."""
    from diffmusic_amd import inverse_problem as P, ops
    from tests.test_gpu_declip import _pipe, _gens, _hand_loop, N_CALL
    B = 3
    pe, clean = _problem(B, LEN)
    op = P.TimeWarpOperator(16000, delay=np.stack([_curve(LEN, seed=b) for b in range(B)]), noiser=P.GaussianNoise(0.0))
    pipe = _pipe(op)
    y = op.forward(clean)
    assert float((y - clean).abs().max()) > 0.05                  # the curve acts
    call = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0)
    got = pipe(generator=_gens(B), output_type="latent", **call).audios
    assert len(pipe.last_losses) == N_CALL and pipe.nan_restarts == 0
    got_losses = [l.reshape(-1).clone() for l in pipe.last_losses]
    x, losses = _hand_loop(pipe, pe, y, B)
    assert torch.equal(got, x)
    assert all(torch.equal(a, b.reshape(-1)) for a, b in zip(got_losses, losses))
    assert all(bool(torch.isfinite(l).all()) and bool((l > 0).all()) for l in got_losses)
    monkeypatch.setattr(ops, "USE_TORCH_OPS", False)
    assert not ops.enabled()
    y_ct = op.forward(clean)
    got_ct = pipe(generator=_gens(B), output_type="latent", **call).audios
    monkeypatch.setattr(ops, "USE_TORCH_OPS", True)
    assert torch.equal(y, y_ct) and torch.equal(got, got_ct)
    with pytest.raises(ValueError, match="per-clip delay curves cannot run as clip lanes"):
        pipe(generator=_gens(B), output_type="latent", lanes=2, **call)


def test_inside_a_track_equals_its_hand_loop():
    from diffmusic_amd import inverse_problem as P
    from tests.test_gpu_declip import _pipe, _gens, _hand_loop, N_CALL
    T, R = 16000, 1600                                       # windows of 6400 at 0, 4800, 9600
    lay = P.TrackLayout(T, LEN, R)
    assert lay.num_windows == 3
    pe, clean = _problem(3, T, seed=21)
    clean = clean[:1].contiguous()
    inner = P.TimeWarpOperator(16000, delay=_curve(T), noiser=P.GaussianNoise(0.0))        # the curve is built for the track's length
    top = P.TrackOperator(inner, lay)
    pipe = _pipe(top, per_clip=False)
    y = top.forward(clean)
    assert y.shape == (1, T) and float((y - clean).abs().max()) > 0.05
    call = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0)
    lat = pipe(generator=_gens(3), output_type="latent", **call).audios
    assert lat.shape == (3, 8, 10, 16) and len(pipe.last_losses) == N_CALL and all(l.numel() == 1 for l in pipe.last_losses)
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
    inner = P.TimeWarpOperator(16000, delay=_curve(LEN), noiser=P.GaussianNoise(0.0))
    top = P.MixtureOperator(inner, K, [1.0, 0.5])
    pipe = _pipe(top)
    y = top.forward(clean)
    assert y.shape == (1, LEN)                                    # the transport acts on the mix
    call = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0)
    lat = pipe(generator=_gens(K), output_type="latent", **call).audios
    assert len(pipe.last_losses) == N_CALL and all(l.numel() == 1 for l in pipe.last_losses)
    got_losses = list(pipe.last_losses)
    _, x, losses = _hand_loop(pipe, pe, y, K)
    assert torch.equal(lat, x)
    assert all(torch.equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(got_losses, losses))
    assert all(bool(torch.isfinite(l).all()) and bool((l > 0).all()) for l in got_losses)


def test_clip_lanes_with_a_shared_curve_equal_the_plain_loop():
    """lanes = 2 on four clips equals the two clip groups run with lanes = 1, bit for bit (a shared curve is no per-clip state), the
    procedure of tests/test_gpu_lanes.py on the small nets."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.pipelines.lanes import split_sizes
    from tests.test_gpu_pipeline import UNET, _build
    B, N = 4, 4
    op = P.TimeWarpOperator(16000, delay=_curve(LEN), noiser=P.GaussianNoise(0.0))
    pipe = _build("musicldm", UNET, "dps", op)
    g = torch.Generator().manual_seed(3)
    pe = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    lat0 = torch.randn(B, 8, 10, 16, generator=g)
    y = op.forward(_clips(B, LEN, 3))

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
