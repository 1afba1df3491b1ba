"""-m gpu: de-compression (csrc/drc.hip, inverse_problem/operator.py DynamicRangeOperator).

Kernel level: every case of tests/drc_cases.py against the float64 model, EVERY element of y, p, s, G and -- given the kernel's own tape --
of dx within the bound derived from the number formats, through both bindings (bit-identical); tape bits differ from the model's only where
the model is ambiguous; a clip alone, in a batch and at another batch position gives the same bits; the NaN rule; refusals.  Operator
level: `apply` / `adjoint` keep the point they were taken at.  Step level: teacher-forced steps against `oracle.schedulers` around an oracle
operator defined here -- torch autograd through the definition -- with the bounds of tests/test_gpu_declip.py.  Call level: `pipe(...)`
equals a hand-written loop bit for bit, alone, inside a TrackOperator and inside a MixtureOperator; clip lanes equal the plain loop."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import drc_cases as D                                                       # noqa: E402
from tests.test_gpu_step import HIFI, VAE, SCHED, H, W as LAT_W, LEN                   # noqa: E402

CANARY = 12345.678
_REPORT = {}


def _bindings():
    from diffmusic_amd import ops
    return (("torch_ops", ops.load()), ("ctypes", ops.ctypes_hip))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _strided(a, off, pad=8):
    """numpy (B, n) -> a GPU view with row stride n + pad whose rows start `off` floats into their slots"""
    B, n = a.shape
    buf = torch.zeros(B, n + pad, dtype=torch.float32, device="cuda")
    view = buf[:, off:off + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return view


def _dev_case(c):
    i = D.inputs(c)
    x = _strided(i.store, c.off)                                   # (B, stride) rows with stride c.stride + 8
    dy = _strided(i.dy, c.off) if c.stride > c.full else torch.from_numpy(i.dy).cuda()
    assert x.stride(0) == c.stride + 8 and x.shape[1] >= c.L
    return i, x, dy


def _run(binding, c, x, dy):
    y, state, tape = binding.drc_fwd(x, c.L, *c.P.args)
    dx = binding.drc_bwd(dy, x, state, tape, c.full, *c.P.args)
    return y, state, tape, dx


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", D.CASES, ids=lambda c: c.name)
def test_kernels_lie_within_the_bound_in_every_element(c):
    i, x, dy = _dev_case(c)
    r, q, rb, qdx = D.reference(c)
    outs = []
    for name, binding in _bindings():
        y, state, tape, dx = _run(binding, c, x, dy)
        assert y.shape == (c.B, c.L) and y.is_contiguous() and state.shape == (c.B, 3, c.H) and tape.shape == (c.B, c.H) and tape.dtype == torch.uint8
        assert dx.shape == (c.B, c.full) and dx.is_contiguous()
        st, tp = state.cpu().numpy(), tape.cpu().numpy()
        got = {"p": D.ratio(st[:, 0], r.p, q.p), "G": D.ratio(st[:, 1], r.G, q.G), "s": D.ratio(st[:, 2], r.s, q.s),
               "y": D.ratio(y.cpu().numpy(), r.y, q.y)}
        flips = int((tp != r.tape).sum())
        assert D.tape_differences_allowed(tp, r, q), (c.name, name, "a tape bit differs where the model is not ambiguous")
        got["dx"] = D.judge_bwd(c, dx[:, :c.L].cpu().numpy(), tp)
        _REPORT[c.name] = max(_REPORT.get(c.name, 0.0), *got.values())
        print(f"\n  {c.name}/{name}: largest |kernel - model| / bound " + " ".join(f"{k} {v:.4f}" for k, v in got.items()) + f"; tape bits flipped {flips}")
        assert all(v <= 1.0 for v in got.values()), (c.name, name, got)
        assert bool((_bits(dx[:, c.L:]) == 0).all()), "dx[:, L:full] is +0.0f"
        outs.append((y, state, tape, dx))
    for a, b in zip(*outs):
        assert torch.equal(_bits(a.float()), _bits(b.float())), "the two bindings are bit-identical"
    if c.signal == "quiet":
        assert not bool(outs[0][2].any()) and not bool(outs[0][1][:, 2].any()), "below the knee: the tape and s are all zero"
        assert bool((outs[0][1][:, 1] == outs[0][1][0, 1, 0]).all()), "one gain for every block"
    if c.signal == "silence":
        assert not bool(outs[0][0].any()) and not bool(outs[0][2].any())


@pytest.mark.parametrize("name", ["L65", "L1000", "L6400_fastrel", "L20037_stride", "L70000"])
def test_a_clip_gives_the_same_bits_alone_in_a_batch_and_at_another_position(name):
    from diffmusic_amd import ops
    c = D.CASE[name]
    i, x, dy = _dev_case(c)
    first = _run(ops.hip, c, x, dy)
    again = _run(ops.hip, c, x, dy)
    for a, b in zip(first, again):
        assert torch.equal(_bits(a.float()), _bits(b.float())), "two runs are bit-equal"
    for b in range(c.B):
        alone = _run(ops.hip, c, x[b:b + 1], dy[b:b + 1])
        for a, f in zip(alone, first):
            assert torch.equal(_bits(a[0].float()), _bits(f[b].float())), (name, b)
    xs, dys = x.flip(0).contiguous(), dy.flip(0).contiguous()     # contiguous rows at the mirrored position: another load path too
    swapped = _run(ops.hip, c, xs, dys)
    for a, f in zip(swapped, first):
        assert torch.equal(_bits(a.flip(0).float()), _bits(f.float())), "neither the batch position nor the load path matters"


def test_a_nan_sample_poisons_its_block_and_what_follows_only():
    """A NaN at sample n of a clip: y is NaN from the first sample of its block to the end of that clip and bit-equal to the clean run
    before it; the state and the tape before that block are the clean ones; every other clip is untouched.  The transpose of that clip is
    NaN throughout (the backward recurrence carries it to the first block), the other clips' is untouched."""
    from diffmusic_amd import ops
    c = D.CASE["L6400"]
    i, x, dy = _dev_case(c)
    clean = _run(ops.hip, c, x, dy)
    n, b = 3000, 1
    j = n // 64
    xn = x.clone()
    xn[b, n] = float("nan")
    for _, binding in _bindings():
        y, state, tape, dx = _run(binding, c, xn, dy)
        assert bool(torch.isnan(y[b, n])) and bool(torch.isnan(y[b, 64 * j:]).all())
        assert torch.equal(_bits(y[b, :64 * j]), _bits(clean[0][b, :64 * j]))
        assert torch.equal(_bits(state[b, :, :j]), _bits(clean[1][b, :, :j])) and torch.equal(tape[b, :j], clean[2][b, :j])
        assert bool(torch.isnan(state[b, 0, j])) and bool(torch.isnan(state[b, 1:, j:]).all())            # p[j]; G and s from block j on
        assert torch.equal(_bits(state[b, 0, j + 1:]), _bits(clean[1][b, 0, j + 1:]))                    # the later blocks' own power
        assert bool(torch.isnan(dx[b, :c.L]).all()) and bool((_bits(dx[b, c.L:]) == 0).all())
        for other in (0, 2):
            for a, f in zip((y, state, tape, dx), clean):
                assert torch.equal(_bits(a[other].float()), _bits(f[other].float())), other


def test_refusals_write_nothing():
    from diffmusic_amd import _lib, ops
    lib = _lib.lib()
    L, full, B = 1500, 1510, 2
    Hn = D.blocks(L)
    x = torch.randn(B, full, device="cuda")
    dy = torch.randn(B, L, device="cuda")
    P = D.PARAMS["base"].args
    y0, state0, tape0 = ops.hip.drc_fwd(x, L, *P)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = C.c_float

    def bufs():
        return [torch.full(s, CANARY, dtype=torch.float32, device="cuda") for s in ((B, L), (B, 3, Hn), (B, Hn), (B, full))] + \
               [torch.full((B, Hn), 77, dtype=torch.uint8, device="cuda")]

    def fwd(xp=x.data_ptr(), xs=full, ys=L, batch=B, L_=L, P_=P, null=None):
        y, state, _, _, tape = bufs()
        ptr = {"y": y.data_ptr(), "state": state.data_ptr(), "tape": tape.data_ptr()}
        if null:
            ptr[null] = 0
        rc = lib.dmx_drc_fwd(C.c_void_p(xp), xs, C.c_void_p(ptr["y"]), ys, C.c_void_p(ptr["state"]), C.c_void_p(ptr["tape"]), batch, L_,
                             *[f(v) for v in P_], st)
        torch.cuda.synchronize()
        return rc, bool((y == CANARY).all() and (state == CANARY).all() and (tape == 77).all())

    def bwd(dyp=dy.data_ptr(), dys=L, xs=full, dxs=full, batch=B, L_=L, full_=full, P_=P, null=None):
        _, _, work, dx, _ = bufs()
        ptr = {"x": x.data_ptr(), "state": state0.data_ptr(), "tape": tape0.data_ptr(), "work": work.data_ptr(), "dx": dx.data_ptr()}
        if null:
            ptr[null] = 0
        rc = lib.dmx_drc_bwd(C.c_void_p(dyp), dys, C.c_void_p(ptr["x"]), xs, C.c_void_p(ptr["state"]), C.c_void_p(ptr["tape"]),
                             C.c_void_p(ptr["work"]), C.c_void_p(ptr["dx"]), dxs, batch, L_, full_, *[f(v) for v in P_], st)
        torch.cuda.synchronize()
        return rc, bool((work == CANARY).all() and (dx == CANARY).all())

    def with_param(k, v):
        p = list(P)
        p[k] = v
        return tuple(p)
    assert fwd() == (0, False) and bwd() == (0, False)            # the same calls with nothing wrong run
    bad_params = [("threshold nan", with_param(0, math.nan)), ("threshold out of range", with_param(0, 1e4)), ("slope > 1", with_param(1, 1.5)),
                  ("slope < 0", with_param(1, -0.1)), ("slope nan", with_param(1, math.nan)), ("knee < 0", with_param(2, -1.0)),
                  ("knee inf", with_param(2, math.inf)), ("attack 0", with_param(3, 0.0)), ("attack > 1", with_param(3, 1.5)),
                  ("release nan", with_param(4, math.nan)), ("makeup inf", with_param(5, math.inf))]
    for what, kw in [("null x", dict(xp=0)), ("null y", dict(null="y")), ("null state", dict(null="state")), ("null tape", dict(null="tape")),
                     ("batch 0", dict(batch=0)), ("batch 65536", dict(batch=65536)), ("L 0", dict(L_=0)), ("short x stride", dict(xs=L - 1)),
                     ("short y stride", dict(ys=L - 1))] + [(w, dict(P_=p)) for w, p in bad_params]:
        rc, untouched = fwd(**kw)
        assert rc != 0 and untouched and lib.dmx_last_error(), ("drc_fwd", what)
    for what, kw in [("null dy", dict(dyp=0)), ("null x", dict(null="x")), ("null state", dict(null="state")), ("null tape", dict(null="tape")),
                     ("null work", dict(null="work")), ("null dx", dict(null="dx")), ("batch 0", dict(batch=0)), ("batch 65536", dict(batch=65536)),
                     ("L 0", dict(L_=0)), ("Lfull < L", dict(full_=L - 1)), ("short dy stride", dict(dys=L - 1)), ("short x stride", dict(xs=L - 1)),
                     ("short dx stride", dict(dxs=full - 1))] + [(w, dict(P_=p)) for w, p in bad_params]:
        rc, untouched = bwd(**kw)
        assert rc != 0 and untouched and lib.dmx_last_error(), ("drc_bwd", what)
    for _, binding in _bindings():                                 # and the bindings' own checks
        with pytest.raises((RuntimeError, AssertionError)):
            binding.drc_fwd(x, full + 1, *P)
        with pytest.raises((RuntimeError, AssertionError)):
            binding.drc_fwd(x, L, *with_param(1, 2.0))
        with pytest.raises((RuntimeError, AssertionError)):
            binding.drc_fwd(x.cpu(), L, *P)
        with pytest.raises((RuntimeError, AssertionError)):
            binding.drc_bwd(dy, x, state0, tape0, L - 1, *P)
        with pytest.raises((RuntimeError, AssertionError)):
            binding.drc_bwd(dy, x, state0[:, :, :-1].contiguous(), tape0, full, *P)
        with pytest.raises((RuntimeError, AssertionError)):
            binding.drc_bwd(dy, x, state0, tape0.float(), full, *P)
        with pytest.raises((RuntimeError, AssertionError)):
            binding.drc_bwd(dy, x[:1], state0, tape0, full, *P)
    assert ops.hip.drc_bwd(dy, x, state0, tape0, full, *P).shape == (B, full)


def test_report_largest_ratios():
    if _REPORT:
        worst = max(_REPORT, key=_REPORT.get)
        print(f"\n  largest |kernel - model| / bound over {len(_REPORT)} cases: {_REPORT[worst]:.4f} ({worst})")


# ---- operator level ---------------------------------------------------------------------------------------------------------------------
def _gated(B, n, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([D.gated_noise(rng, n) for _ in range(B)]).astype(np.float32)).cuda()


def test_apply_and_adjoint_keep_the_point_they_were_taken_at():
    """The contract of tests/test_gpu_operator_contract.py::test_the_declipping_transpose_keeps_the_point_it_was_taken_at: the closure holds x,
    the state and the tape of ITS apply; a later apply on another input changes nothing.  And forward = apply + the noiser."""
    from diffmusic_amd import inverse_problem as P, ops
    length, pad, B = 6400, 32, 2
    op = P.DynamicRangeOperator(16000)
    x = _gated(B, length + pad, 4)
    y, adjoint = op.apply(x, length)
    y_k, state, tape = ops.hip.drc_fwd(x, length, *op.params)
    assert torch.equal(y, y_k) and y.shape == (B, length)
    share = float(((tape & 3) == 2).float().mean())
    assert 0.05 < share < 0.95, share                             # both sides of the threshold
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).cuda()
    want = ops.hip.drc_bwd(w, x, state, tape, length + pad, *op.params)
    got = adjoint(w, length + pad)
    assert got.shape == x.shape and torch.equal(got, want) and float(got[:, length:].abs().max()) == 0.0
    x2 = _gated(B, length + pad, 6)
    y2, adjoint2 = op.apply(x2, length)
    assert not torch.equal(ops.hip.drc_fwd(x2, length, *op.params)[2], tape)
    assert torch.equal(adjoint(w, length + pad), want)            # the first call's transpose, after the second call
    assert not torch.equal(adjoint2(w, length + pad), want)
    assert torch.equal(op.forward(x[:, :length].contiguous()), y)
    fixed = torch.randn(B, length, generator=torch.Generator().manual_seed(4)).cuda()
    op.noiser = lambda v: v + 0.1 * fixed
    assert torch.equal(op.forward(x[:, :length].contiguous()), y + 0.1 * fixed)
    # <J^T w, v> against a directional difference of A in fp32: a coarse check that the closure is the transpose at x (the exact one is
    # the element-wise test above)
    v = torch.randn(x.shape, generator=torch.Generator().manual_seed(8)).cuda()
    v[:, length:] = 0
    h = 1e-3
    op.noiser = None
    fd = (op.apply(x + h * v, length)[0].double() - op.apply(x - h * v, length)[0].double()) / (2 * h)
    lhs, rhs = float((w.double() * fd).sum()), float((got.double() * v.double()).sum())
    assert abs(lhs - rhs) <= 2e-2 * max(abs(lhs), abs(rhs)), (lhs, rhs)


@pytest.mark.parametrize("space", ["wav_form", "mel_spectrogram"])
def test_guidance_is_the_composition_of_its_parts(space, monkeypatch):
    from diffmusic_amd import inverse_problem as P, ops
    from tests.test_gpu_operator_contract import _chain
    length, pad, B = 6400, 32, 2
    op = P.DynamicRangeOperator(16000, noiser=P.GaussianNoise(0.0))
    wav, clean = _gated(B, length + pad, 1), _gated(B, length, 2)
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
def torch_drc(x, P):
    """The definition in torch, differentiable: x (B, L) -> y (B, L); P as `D.params` returns it."""
    B, L = x.shape
    Hn = D.blocks(L)
    xb = torch.nn.functional.pad(x, (0, Hn * 64 - L)).reshape(B, Hn, 64)
    p = (xb * xb).sum(-1) / 64
    d = 10.0 * torch.log10(p + D.EPS) - P.T
    t = d + 0.5 * P.W
    c = torch.where(2.0 * d < -P.W, torch.zeros_like(d), torch.where(2.0 * d <= P.W, P.kq * t * t, P.k * d))
    s, rows = torch.zeros(B, dtype=x.dtype), []
    for j in range(Hn):
        a = torch.where(c[:, j] > s, torch.full_like(s, P.aA), torch.full_like(s, P.aR))
        s = s + a * (c[:, j] - s)
        rows.append(s)
    s = torch.stack(rows, dim=1)
    G = 10.0 ** ((P.makeup - s) / 20.0)
    Gp = torch.cat([torch.full((B, 1), 10.0 ** (P.makeup / 20.0), dtype=x.dtype), G[:, :-1]], dim=1)
    w = (torch.arange(64, dtype=x.dtype) + 1.0) / 64
    g = (Gp[..., None] + w * (G - Gp)[..., None]).reshape(B, Hn * 64)[:, :L]
    return g * x


def _oracle_drc(sample_rate, P, noiser=None):
    from oracle import audio, operators as O

    class OracleDrc(O.BaseOperator):
        def __init__(self):
            self.wav2mel = audio.Wav2Mel(sample_rate)
            self.noiser = noiser

        def transform(self, a):
            return torch.clamp(self.wav2mel(a), min=-80, max=80)

        def forward(self, data, **k):
            y = torch_drc(data, P)
            return self.noiser(y) if self.noiser is not None else y
    return OracleDrc()


class _FixedNoiser:
    def __init__(self, sigma, z):
        self.sigma, self.z = sigma, z

    def __call__(self, data):
        return data + self.sigma * self.z


def test_torch_restatement_agrees_with_the_float64_model():
    for name in ("L1000", "L6400_hard", "L6400_fastrel"):
        c = D.CASE[name]
        i = D.inputs(c)
        r, _, rb, _ = D.reference(c)
        x = torch.from_numpy(i.x.copy()).double().requires_grad_(True)
        y = torch_drc(x, c.P)
        (gx,) = torch.autograd.grad((y * torch.from_numpy(i.dy).double()).sum(), x)
        assert np.abs(y.detach().numpy() - r.y).max() <= 1e-12 * max(1.0, np.abs(r.y).max())
        assert np.abs(gx.numpy() - rb.dx).max() <= 1e-11 * max(1.0, np.abs(rb.dx).max())


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


def _block_levels(wav):
    B, L = wav.shape
    Hn = D.blocks(L)
    xb = torch.nn.functional.pad(wav.double(), (0, Hn * 64 - L)).reshape(B, Hn, 64)
    return 10.0 * torch.log10((xb * xb).sum(-1) / 64 + D.EPS)


STEP_CASES = [("dps", 0.0, 5e-4, "mel_spectrogram", 501, True, 0.0), ("dps", 0.0, 5e-4, "wav_form", 996, True, 0.0),
              ("mpgd", 0.0, 5e-3, "mel_spectrogram", 251, True, 0.0), ("dsg", 1.0, 0.08, "mel_spectrogram", 501, False, 0.0),
              ("dps", 0.0, 5e-4, "mel_spectrogram", 501, True, 0.05)]


@pytest.mark.parametrize("name,eta,rate,space,t,per_clip,sigma", STEP_CASES,
                         ids=[f"{c[0]}-{c[3]}-{'clip' if c[5] else 'batch'}-sigma{c[6]}" for c in STEP_CASES])
def test_teacher_forced_decompression_step(nets, name, eta, rate, space, t, per_clip, sigma):
    """The procedure and the bounds of tests/test_gpu_declip.py::test_teacher_forced_declipping_step: forward < 1e-4, loss < 1e-2, gradient
    cosine > 0.98, prev_sample < 1e-2.  The threshold is the median block level of the ORACLE's predicted waveform rvoc(rvae(x0_hat)), so
    half of the oracle's blocks lie above it by construction; the product's share above the threshold must lie in (0.02, 0.98)."""
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
    rs = OS.get_scheduler(name)(operator=None, per_clip_norm=per_clip, **SCHED)
    rs.set_timesteps(200)
    with torch.no_grad():
        _, x0 = rs.parent_step(e, t, x, 0.0, None, None)
        wav_o = rvoc(rvae.decode(x0 / VAE["scaling_factor"]).sample.squeeze(1))[:, :LEN]
    thr = float(_block_levels(wav_o).median())                  # on the CPU, from the oracle's prediction
    op = P.DynamicRangeOperator(16000, threshold_db=thr, noiser=None)
    par = D.params(threshold_db=op.threshold_db)
    assert par.args == op.params
    rop = _oracle_drc(16000, par)
    y_clean = rop.forward(clean)
    rf = _rel(op.forward(clean.cuda()), y_clean)
    print(f"\n  operator.forward rel-L2 {rf:.2e}")
    assert rf < 1e-4, "operator.forward"
    rop.noiser = _FixedNoiser(sigma, z_meas) if sigma > 0 else None
    y_ref = rop.forward(clean)
    y = y_ref.cuda()
    op.noiser = P.GaussianNoise(sigma)
    seen = {}
    inner = op.guidance

    def spy(wav, length, *a, **k):
        seen["wav"] = wav[:, :length].detach().clone()
        return inner(wav, length, *a, **k)
    op.guidance = spy
    sched = get_scheduler(name)(operator=op, per_clip_norm=per_clip, **SCHED)
    sched.set_timesteps(200)
    sched.debug_keep_grad = True
    rs.operator = rop
    rop.noiser = _FixedNoiser(sigma, z_step) if sigma > 0 else None
    kw = dict(eta=eta, ip_guidance_rate=rate, original_waveform_length=LEN, supervised_space=space)
    noise_kw = dict(sample_noise=z.cuda()) if name == "dsg" else dict(variance_noise=None)
    opk = dict(noise=z_step.cuda()) if sigma > 0 else {}
    out = sched.step(e.cuda(), t, x.cuda(), measurement=y, vae=vae, vocoder=voc, op_kwargs=opk, **kw, **noise_kw)
    torch.cuda.synchronize()
    rnoise = dict(sample_noise=z) if name == "dsg" else dict(variance_noise=None)
    ro = rs.step(e, t, x, measurement=y_ref, vae=rvae, vocoder=rvoc, **kw, **rnoise)
    share_p = float((_block_levels(seen["wav"].cpu()) > par.T).double().mean())
    share_o = float((_block_levels(wav_o) > par.T).double().mean())
    rp = _rel(out.prev_sample, ro.prev_sample)
    rl = _rel(out.loss.reshape(-1), ro.loss.reshape(-1))
    rgr = _rel(sched.last_grad, ro.sample)
    cos = torch.nn.functional.cosine_similarity(sched.last_grad.cpu().flatten(), ro.sample.flatten(), dim=0).item()
    msg = (f"drc {name}/{space}/{'clip' if per_clip else 'batch'}/sigma={sigma}: T {thr:.2f} dB prev {rp:.2e} loss {rl:.2e} grad {rgr:.2e} "
           f"cos {cos:.4f} blocks above threshold product {share_p:.3f} oracle {share_o:.3f}")
    print("\n  " + msg)
    assert 0.02 < share_p < 0.98, msg
    assert abs(share_o - 0.5) < 0.02, msg
    assert _rel(out.pred_original_sample, ro.pred_original_sample) < 1e-4 or name == "mpgd"
    assert rl < 1e-2, msg
    assert cos > 0.98, msg
    assert rp < 1e-2, msg


# ---- call level -----------------------------------------------------------------------------------------------------------------------
SECONDS = 0.4


def _problem(B, T, seed=11):
    g = torch.Generator().manual_seed(seed)
    pe = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    return pe, _gated(B, T, seed) * 0.6


def test_call_equals_the_hand_written_loop(monkeypatch):
    """`pipe(...)` with a DynamicRangeOperator against `_unet_eps` + `scheduler.step` written out: bit for bit, latents and losses; the ctypes
    binding gives the same bits."""
    from diffmusic_amd import inverse_problem as P, ops
    from tests.test_gpu_declip import _pipe, _gens, _hand_loop, N_CALL
    B = 3
    pe, clean = _problem(B, LEN)
    op = P.DynamicRangeOperator(16000, threshold_db=-30.0, ratio=math.inf, noiser=P.GaussianNoise(0.0))
    pipe = _pipe(op)
    y = op.forward(clean)
    assert float((y - clean).abs().max()) > 0.05                  # the limiter acts
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


def test_inside_a_track_equals_its_hand_loop():
    from diffmusic_amd import inverse_problem as P
    from tests.test_gpu_declip import _pipe, _gens, _hand_loop, N_CALL
    T, R = 16000, 1600                                       # windows of 6400 at 0, 4800, 9600
    lay = P.TrackLayout(T, LEN, R)
    assert lay.num_windows == 3
    pe, clean = _problem(3, T, seed=21)
    clean = clean[:1].contiguous()
    inner = P.DynamicRangeOperator(16000, noiser=P.GaussianNoise(0.0))
    top = P.TrackOperator(inner, lay)
    pipe = _pipe(top, per_clip=False)
    y = top.forward(clean)
    assert y.shape == (1, T) and float((y - clean).abs().max()) > 0.01           # the follower runs over the whole track
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
    inner = P.DynamicRangeOperator(16000, noiser=P.GaussianNoise(0.0))
    top = P.MixtureOperator(inner, K, [1.0, 0.5])
    pipe = _pipe(top)
    y = top.forward(clean)
    assert y.shape == (1, LEN)                                    # the bus compressor acts on the mix
    call = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0)
    lat = pipe(generator=_gens(K), output_type="latent", **call).audios
    assert len(pipe.last_losses) == N_CALL and all(l.numel() == 1 for l in pipe.last_losses)
    got_losses = list(pipe.last_losses)
    _, x, losses = _hand_loop(pipe, pe, y, K)
    assert torch.equal(lat, x)
    assert all(torch.equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(got_losses, losses))
    assert all(bool(torch.isfinite(l).all()) and bool((l > 0).all()) for l in got_losses)


def test_clip_lanes_equal_the_plain_loop():
    """lanes = 2 on four clips equals the two clip groups run with lanes = 1, bit for bit (the operator keeps nothing per clip), the
    procedure of tests/test_gpu_lanes.py on the small nets."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.pipelines.lanes import split_sizes
    from tests.test_gpu_pipeline import UNET, _build
    B, N = 4, 4
    op = P.DynamicRangeOperator(16000, noiser=P.GaussianNoise(0.0))
    pipe = _build("musicldm", UNET, "dps", op)
    g = torch.Generator().manual_seed(3)
    pe = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    lat0 = torch.randn(B, 8, 10, 16, generator=g)
    y = op.forward(_gated(B, LEN, 3) * 0.6)

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
