"""-m gpu: blind de-compression (csrc/drc.hip's table route, csrc/drc_fit.hip, BlindDynamicRangeOperator).

Kernel level: every case of tests/drc_fit_cases.py against the float64 models, EVERY element of y, s, G, dx, the partial rows and the
updated phi, moments and table within the bound derived from the number formats, through both bindings (bit-identical); tape differences
only where the model is ambiguous; the table route bit-equal to the host-scalar route on a uniform table; a clip's bits alone, in a batch
and at another batch position; a NaN clip and a non-finite table row stay in their clip and keep their state; refusals through the C ABI.
Operator level: a frozen or pinned estimate equals DynamicRangeOperator bit for bit, one live step in each supervised space against torch
autograd through the definition, reset / restart, and 400 steps on fixed gated noise recover known compressor settings.  Call level: the
pipeline runs it deterministically, under both bindings, inside a track and inside a mixture, and refuses lanes and shards by name."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import drc_cases as D                                                       # noqa: E402
from tests import drc_fit_cases as F                                                   # noqa: E402
from tests.test_drc_fit_bound_host import _torch_forward                               # noqa: E402
from tests.test_gpu_step import HIFI, VAE, SCHED, H, W as LAT_W, LEN                   # noqa: E402

CANARY = 12345.678
_REPORT = {}
f64 = np.float64


def _bindings():
    from diffmusic_amd import ops
    return (("torch_ops", ops.load()), ("ctypes", ops.ctypes_hip))


def _bits(t):
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b))


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _dev_case(c):
    """the case's x as a view with the case's row stride and offset (canaries around the rows), dy and the table"""
    i = F.inputs(c)
    buf = torch.full((c.B, c.stride + 8), CANARY, dtype=torch.float32, device="cuda")
    buf[:, :c.stride] = torch.from_numpy(i.store)
    x = buf[:, c.off:c.off + c.L]
    assert x.stride(0) == c.stride + 8
    return i, x, torch.from_numpy(i.dy).cuda(), torch.from_numpy(i.theta).cuda()


def _chain(binding, c, x, dy, theta):
    """drc_fwd_p, drc_bwd_p, drc_pgrad of one binding -> (y, state, tape, dx, work, bq0, part)"""
    y, state, tape = binding.drc_fwd_p(x, c.L, theta, c.W)
    dx, work, bq0 = binding.drc_bwd_p(dy, x, state, tape, theta, c.full, c.W)
    part = binding.drc_pgrad(state, tape, work, bq0, theta, c.L, c.W)
    return y, state, tape, dx, work, bq0, part


def _update(binding, c, part):
    u = F.update_setup(c)
    st = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (u.phi, u.m, u.v, u.theta)]
    binding.drc_update(part, *st, c.L, u.k, list(u.lr), F.BETAS[0], F.BETAS[1], F.ADAM_EPS, c.W, list(u.lo), list(u.hi))
    return st


# ---- kernel level: every element ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", F.CASES, ids=lambda c: c.name)
def test_every_element_lies_within_the_bound(c):
    i, x, dy, theta = _dev_case(c)
    outs = []
    for name, binding in _bindings():
        y, state, tape, dx, work, bq0, part = out = _chain(binding, c, x, dy, theta)
        assert y.shape == (c.B, c.L) and state.shape == (c.B, 3, c.H) and tape.shape == (c.B, c.H) and dx.shape == (c.B, c.full)
        assert work.shape == (c.B, 2, c.H) and bq0.shape == (c.B,) and part.shape == (c.B, c.nseg, 5) and part.is_contiguous()
        assert not dx[:, c.L:].any(), "zeros past L"
        yn, sn, tn, dxn = y.cpu().numpy(), state.cpu().numpy(), tape.cpu().numpy(), dx.cpu().numpy()
        worst = {}
        for b in range(c.B):
            r, q = F.forward(c)[b]
            assert D.tape_differences_allowed(tn[b:b + 1], r, q), (c.name, name, b)
            assert D.ambiguous_share(q) <= (D.AMBIG_CAP if c.H >= 100 else 0.0)              # the condition of the line above
            rb, qdx, _, _ = F.backward(c, b, tn[b])
            for key, got, want, bnd in (("y", yn[b], r.y[0], q.y[0]), ("s", sn[b, 2], r.s[0], q.s[0]), ("G", sn[b, 1], r.G[0], q.G[0]),
                                        ("p", sn[b, 0], r.p[0], q.p[0]), ("dx", dxn[b, :c.L], rb.dx[0], qdx[0])):
                worst[key] = max(worst.get(key, 0.0), F.ratio(got, want, bnd))
        pn = part.cpu().numpy()
        worst["part"] = F.judge_pgrad(c, pn, [tn[b] for b in range(c.B)])
        st = _update(binding, c, part)
        worst["update"] = F.judge_update(c, pn, [t.cpu().numpy() for t in st])
        _REPORT[c.name] = max(_REPORT.get(c.name, 0.0), max(worst.values()))
        print(f"\n  {c.name}/{name}: largest |kernel - model| / bound: " + "  ".join(f"{k} {v:.4f}" for k, v in worst.items()))
        assert max(worst.values()) <= 1.0, (c.name, name, worst)
        outs.append(list(out) + st)
    assert _same(outs[0], outs[1]), "the two bindings are bit-identical"
    if c.name == "L6400_quiet_clip":
        part = outs[0][6]
        assert not part[2][:, [0, 1, 3, 4]].any() and bool(part[2][:, 2].any()) and not outs[0][2][2].any()


def test_report_largest_ratios():
    if _REPORT:
        worst = max(_REPORT, key=_REPORT.get)
        print(f"\n  largest |kernel - model| / bound over {len(_REPORT)} cases: {_REPORT[worst]:.4f} ({worst})")


@pytest.mark.parametrize("name", ["L65", "L1000", "L6400_hard", "L6400_limiter", "L20037_stride", "L70000"])
def test_uniform_table_is_bit_equal_to_the_host_scalar_route(name):
    from diffmusic_amd import ops
    from diffmusic_amd.inverse_problem import dsp
    c = F.CASE[name]
    i, x, dy, _ = _dev_case(c)
    for P in c.P[:2]:
        theta = torch.from_numpy(dsp.drc_table(P.T, P.k, P.aA, P.aR, P.makeup, c.W, c.B)).cuda()
        y, state, tape = ops.hip.drc_fwd(x, c.L, *P.args)
        dx = ops.hip.drc_bwd(dy, x, state, tape, c.full, *P.args)
        yp, statep, tapep = ops.hip.drc_fwd_p(x, c.L, theta, c.W)
        dxp, work, bq0 = ops.hip.drc_bwd_p(dy, x, statep, tapep, theta, c.full, c.W)
        assert _same((y, state, tape, dx), (yp, statep, tapep, dxp)), name
        assert bool(torch.isfinite(work).all()) and bool(torch.isfinite(bq0).all())


@pytest.mark.parametrize("name", ["L65", "L1000", "L20037_stride", "L70000"])
def test_a_clip_gives_the_same_bits_alone_in_a_batch_and_at_another_position(name):
    from diffmusic_amd import ops
    c = F.CASE[name]
    i, x, dy, theta = _dev_case(c)
    whole = _chain(ops.hip, c, x, dy, theta)
    assert _same(whole, _chain(ops.hip, c, x, dy, theta))
    alone = _chain(ops.hip, c, x[2:3].clone(), dy[2:3].contiguous(), theta[2:3].contiguous())       # position 0 of 1, a contiguous row
    assert _same([t[0] for t in alone], [t[2] for t in whole])
    order = [2, 0, 1]
    moved = _chain(ops.hip, c, x[order].contiguous(), dy[order].contiguous(), theta[order].contiguous())
    assert all(_same([t[k] for t in moved], [t[b] for t in whole]) for k, b in enumerate(order))
    st_whole, st_moved = _update(ops.hip, c, whole[6]), None
    u = F.update_setup(c)
    st_moved = [torch.from_numpy(np.ascontiguousarray(a[order])).cuda() for a in (u.phi, u.m, u.v, u.theta)]
    ops.hip.drc_update(moved[6], *st_moved, c.L, u.k, list(u.lr), F.BETAS[0], F.BETAS[1], F.ADAM_EPS, c.W, list(u.lo), list(u.hi))
    assert all(_same([t[k] for t in st_moved], [t[b] for t in st_whole]) for k, b in enumerate(order))


@pytest.mark.parametrize("what", ["x", "dy", "row_nan", "row_inf"])
def test_a_nan_clip_and_a_non_finite_row_stay_in_their_clip_and_keep_their_state(what):
    from diffmusic_amd import ops
    c = F.CASE["L20037_stride"]
    i, x, dy, theta = _dev_case(c)
    clean = _chain(ops.hip, c, x, dy, theta)
    if what == "x":
        x[1, 5000] = float("nan")
    elif what == "dy":
        dy[1, 5000] = float("nan")
    else:
        theta[1, 0 if what == "row_inf" else 6] = float("inf") if what == "row_inf" else float("nan")
    bad = _chain(ops.hip, c, x, dy, theta)
    for b in (0, 2):
        assert _same([t[b] for t in bad], [t[b] for t in clean]), "the other clips keep their bits"
    y, state, tape, dx, work, bq0, part = bad
    if what.startswith("row"):
        assert bool(torch.isnan(y[1]).all()) and bool(torch.isnan(state[1, 1:]).all()), "NaN from block 0 on"
    if what == "x":
        j = 5000 // 64
        assert torch.equal(_bits(y[1, :64 * j]), _bits(clean[0][1, :64 * j])) and bool(torch.isnan(y[1, 64 * j:]).all())
    if what != "dy":
        assert bool(torch.isnan(dx[1, :c.L]).all())
    assert bool(torch.isnan(part[1]).any())
    st = _update(ops.hip, c, part)
    u = F.update_setup(c)
    ref = _update(ops.hip, c, clean[6])
    for t, t0, tr in zip(st, (u.phi, u.m, u.v, u.theta), ref):
        assert torch.equal(_bits(t[1]), _bits(torch.from_numpy(np.ascontiguousarray(t0[1])).cuda())), "the clip keeps its whole state"
        assert torch.equal(_bits(t[0]), _bits(tr[0])) and torch.equal(_bits(t[2]), _bits(tr[2]))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi_write_nothing():
    """Argument checks only: every refused call returns the shape error before anything is launched."""
    from diffmusic_amd import _lib
    from diffmusic_amd.inverse_problem import dsp
    lib = _lib.lib()
    L, B = 1500, 2
    Hh, n = D.blocks(L), F.segments(D.blocks(L))
    x, dy = torch.randn(B, L + 10, device="cuda"), torch.randn(B, L, device="cuda")
    theta = torch.from_numpy(dsp.drc_table(-24.0, 0.75, 0.5, 0.1, 0.0, 6.0, B)).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = C.c_void_p

    def canary(k):
        return torch.full((k,), CANARY, dtype=torch.float32, device="cuda")
    good_state, good_tape = torch.empty(B, 3, Hh, device="cuda"), torch.empty(B, Hh, dtype=torch.uint8, device="cuda")
    y0 = torch.empty(B, L, device="cuda")
    assert lib.dmx_drc_fwd_p(p(x.data_ptr()), L + 10, p(y0.data_ptr()), L, p(good_state.data_ptr()), p(good_tape.data_ptr()), p(theta.data_ptr()),
                             B, L, 6.0, st) == 0

    def fwd(xs=L + 10, L_=L, B_=B, W=6.0, tp=theta.data_ptr(), xp=x.data_ptr()):
        buf = canary(B * L + B * 3 * Hh + B * Hh)
        rc = lib.dmx_drc_fwd_p(p(xp), xs, p(buf.data_ptr()), L_, p(buf[B * L:].data_ptr()), p(buf[B * L + B * 3 * Hh:].data_ptr()), p(tp), B_, L_, W, st)
        torch.cuda.synchronize()
        return rc, bool((buf == CANARY).all())

    def bwd(W=6.0, tp=theta.data_ptr(), bq_null=False, B_=B, full=L):
        buf = canary(B * 2 * Hh + B + B * L)
        rc = lib.dmx_drc_bwd_p(p(dy.data_ptr()), L, p(x.data_ptr()), L + 10, p(good_state.data_ptr()), p(good_tape.data_ptr()), p(tp),
                               p(buf.data_ptr()), p(0 if bq_null else buf[B * 2 * Hh:].data_ptr()), p(buf[B * 2 * Hh + B:].data_ptr()), L, B_, L,
                               full, W, st)
        torch.cuda.synchronize()
        return rc, bool((buf == CANARY).all())
    assert fwd()[0] == 0 and not fwd()[1] and bwd()[0] == 0 and not bwd()[1]          # the same calls with nothing wrong run
    for what, kw in (("null table", dict(tp=0)), ("W < 0", dict(W=-1.0)), ("W > 200", dict(W=200.5)), ("W nan", dict(W=float("nan"))),
                     ("short x stride", dict(xs=L - 1)), ("L < 1", dict(L_=0)), ("batch 0", dict(B_=0)), ("B > 65535", dict(B_=65536)),
                     ("null x", dict(xp=0))):
        rc, untouched = fwd(**kw)
        assert rc != 0 and untouched and lib.dmx_last_error(), what
    for what, kw in (("null table", dict(tp=0)), ("W < 0", dict(W=-1.0)), ("W inf", dict(W=float("inf"))), ("null bq0", dict(bq_null=True)),
                     ("batch 0", dict(B_=0)), ("Lfull < L", dict(full=L - 1))):
        rc, untouched = bwd(**kw)
        assert rc != 0 and untouched and lib.dmx_last_error(), what
    work, bq0 = torch.zeros(B, 2, Hh, device="cuda"), torch.zeros(B, device="cuda")

    def pgrad(W=6.0, tp=theta.data_ptr(), wp=work.data_ptr(), B_=B, L_=L):
        buf = canary(B * n * 5 + 16)
        rc = lib.dmx_drc_pgrad(p(good_state.data_ptr()), p(good_tape.data_ptr()), p(wp), p(bq0.data_ptr()), p(tp), p(buf.data_ptr()), B_, L_, W, st)
        torch.cuda.synchronize()
        return rc, bool((buf == CANARY).all())
    good_state.zero_(), good_tape.zero_()
    assert pgrad() == (0, False)
    for what, kw in (("null table", dict(tp=0)), ("null work", dict(wp=0)), ("W < 0", dict(W=-0.5)), ("batch 0", dict(B_=0)), ("L 0", dict(L_=0))):
        rc, untouched = pgrad(**kw)
        assert rc != 0 and untouched and lib.dmx_last_error(), what
    part = torch.full((B, n, 5), 0.01, device="cuda")
    five = C.c_double * 5
    box = (five(-60, 0, -24, -6, -6), five(0, 1, 24, 0, 0))

    def update(k=1, lr=(0.25, 0.01, 0.1, 0.02, 0.02), b1=0.9, b2=0.999, eps=1e-8, W=6.0, lo=box[0], hi=box[1], B_=B, pp=part.data_ptr(),
               th_null=False):
        state = canary(3 * B * 5 + B * 8)
        ptr = [state[i * B * 5:].data_ptr() for i in range(3)] + [state[3 * B * 5:].data_ptr()]
        rc = lib.dmx_drc_update(p(pp), p(ptr[0]), p(ptr[1]), p(ptr[2]), p(0 if th_null else ptr[3]), B_, L, k, five(*lr), b1, b2, eps, W, lo, hi, st)
        torch.cuda.synchronize()
        return rc, bool((state == CANARY).all())
    assert update() == (0, False) and update(lr=(0.25, 0, 0, 0, 0)) == (0, False)
    for what, kw in (("k < 1", dict(k=0)), ("lr < 0", dict(lr=(0.25, -0.01, 0.1, 0.02, 0.02))), ("lr nan", dict(lr=(float("nan"), 0, 0, 0, 0))),
                     ("beta1 = 1", dict(b1=1.0)), ("beta2 < 0", dict(b2=-0.1)), ("eps < 0", dict(eps=-1e-8)), ("W < 0", dict(W=-1.0)),
                     ("k box above 1", dict(hi=five(0, 1.5, 24, 0, 0))), ("k box below 0", dict(lo=five(-60, -0.1, -24, -6, -6))),
                     ("ln a above 0", dict(hi=five(0, 1, 24, 0.1, 0))), ("ln a below -80", dict(lo=five(-60, 0, -24, -90, -6))),
                     ("T box beyond 200", dict(lo=five(-300, 0, -24, -6, -6))), ("lo > hi", dict(lo=five(1, 0, -24, -6, -6))),
                     ("batch 0", dict(B_=0)), ("null part", dict(pp=0)), ("null theta", dict(th_null=True))):
        rc, untouched = update(**kw)
        assert rc != 0 and untouched and lib.dmx_last_error(), what
    for _, binding in _bindings():                                 # and the bindings' own checks
        with pytest.raises((RuntimeError, AssertionError)):
            binding.drc_fwd_p(x, L, theta[:1].contiguous(), 6.0)
        with pytest.raises((RuntimeError, AssertionError)):
            binding.drc_fwd_p(x, L, theta, -1.0)
        with pytest.raises((RuntimeError, AssertionError)):
            binding.drc_pgrad(good_state, good_tape, work[:, :1].contiguous(), bq0, theta, L, 6.0)
        with pytest.raises((RuntimeError, AssertionError)):
            binding.drc_update(part, *[torch.zeros(B, 5, device="cuda") for _ in range(3)], theta.clone(), L, 1, [0.1] * 4, 0.9, 0.999, 1e-8, 6.0,
                               list(box[0]), list(box[1]))


# ---- operator level -----------------------------------------------------------------------------------------------------------------------
TRUE = dict(F.REC_TRUE)
START = dict(threshold_db=-18.0, ratio=2.0, attack_ms=5.0, release_ms=100.0, makeup_db=0.0)
ALL = ("threshold", "ratio", "makeup", "attack", "release")


def _clip_pair(seed=77):
    g = torch.Generator().manual_seed(seed)
    clean = torch.from_numpy(np.stack([D.gated_noise(np.random.default_rng(seed + b), LEN) for b in range(2)])).float()
    wav = torch.nn.functional.pad(clean + 0.02 * torch.randn(2, LEN, generator=g), (0, 32))     # a vocoder output: LEN + 32 samples
    return clean, wav


def _blind(**kw):
    from diffmusic_amd import inverse_problem as P
    kw.setdefault("init", START)
    kw.setdefault("fit", ALL)
    return P.BlindDynamicRangeOperator(**kw)


@pytest.mark.parametrize("sigma", [0.0, 0.05])
@pytest.mark.parametrize("space", ["wav_form", "mel_spectrogram"])
def test_frozen_estimate_equals_the_fixed_parameter_operator(space, sigma):
    from diffmusic_amd import inverse_problem as P, ops
    clean, wav = _clip_pair()
    blind = _blind()
    y = blind.forward(clean.cuda(), params=TRUE)
    assert torch.equal(y, P.DynamicRangeOperator(16000, knee_db=6.0, **TRUE).forward(clean.cuda())) and blind.true_params == TRUE
    assert torch.equal(blind.forward(clean.cuda()), y)                                # the kept parameters serve the next call
    wd = wav.cuda()
    out, _ = blind.apply(wd, LEN)                                                      # fixes the batch: the state exists
    phi0, th0 = blind.phi_estimate.clone(), blind.table_estimate.clone()
    assert torch.equal(out, ops.hip.drc_fwd_p(wd, LEN, th0, 6.0)[0])
    est = blind.drc_estimate
    assert est.shape == (2, 5) and np.allclose(est, [[-18.0, 2.0, 0.0, 5.0, 100.0]] * 2, rtol=1e-5, atol=1e-6)
    known = P.DynamicRangeOperator(16000, knee_db=6.0, **START)
    blind.noiser, known.noiser = P.GaussianNoise(sigma), P.GaussianNoise(sigma)
    z = torch.randn(2, LEN, generator=torch.Generator().manual_seed(3)).cuda()
    nk = dict(noise=z) if sigma > 0 else {}
    loss, dwav = blind.guidance(wd, LEN, y, space, update_drc=False, **nk)
    rloss, rdwav = known.guidance(wd, LEN, y, space, **nk)
    assert torch.equal(_bits(loss), _bits(rloss)) and torch.equal(_bits(dwav), _bits(rdwav)) and dwav.shape == wd.shape
    assert bool(dwav.abs().max() > 0) and not dwav[:, LEN:].any()
    loss2, dwav2 = blind.guidance(wd, LEN, y, space, params=START, **nk)               # pinned parameters never update either
    assert torch.equal(loss2, rloss) and torch.equal(dwav2, rdwav)
    assert blind.k == 0 and torch.equal(_bits(blind.phi_estimate), _bits(phi0)) and torch.equal(_bits(blind.table_estimate), _bits(th0))
    assert not blind._m.any() and not blind._v.any()
    live_loss, live_dwav = blind.guidance(wd, LEN, y, space, **nk)                     # a live step takes its gradient at phi_0, then moves phi
    assert torch.equal(live_loss, rloss) and torch.equal(live_dwav, rdwav) and blind.k == 1
    assert not torch.equal(blind.phi_estimate, phi0) and not torch.equal(blind.table_estimate, th0)


@pytest.mark.parametrize("space", ["wav_form", "mel_spectrogram"])
def test_one_live_step_against_autograd_through_the_definition(space):
    """One live guided step; the loss, the x-gradient and the parameter gradient against torch autograd through the float64 restatement
    of the recurrence -> (mel) -> L2, under the bounds tests/test_gpu_blind_time_warp.py holds its live steps to: loss < 1e-2 relative,
    gradient cosine > 0.98.  The kernel's parameter gradient is read from the first moment after the first update, m = (1 - beta1) g."""
    from oracle import audio
    clean, wav = _clip_pair()
    blind = _blind()
    y = blind.forward(clean.cuda(), params=TRUE)
    wd = wav.cuda()
    loss, dwav = blind.guidance(wd, LEN, y, space)
    assert blind.k == 1
    g = blind._m.double().cpu() / float(np.float32(1.0 - 0.9))
    phi = torch.tensor(F.rows_phi([START] * 2), dtype=torch.float64, requires_grad=True)
    xs = wav[:, :LEN].double().requires_grad_(True)
    pred = torch.stack([_torch_forward(xs[b], LEN, phi[b], 6.0) for b in range(2)])
    ref = y.double().cpu()
    if space == "mel_spectrogram":
        wav2mel = audio.Wav2Mel(16000)
        pred, ref = (torch.clamp(wav2mel(t.float()), min=-80, max=80).reshape(2, -1) for t in (pred, ref))
    rloss = torch.linalg.norm(ref - pred, dim=1)
    rg, rdx = torch.autograd.grad(rloss.sum(), (phi, xs))
    cos_p = torch.nn.functional.cosine_similarity(g.flatten(), rg.double().flatten(), dim=0).item()
    cos_x = torch.nn.functional.cosine_similarity(dwav[:, :LEN].double().cpu().flatten(), rdx.double().flatten(), dim=0).item()
    rl = _rel(loss.reshape(-1), rloss.detach())
    print(f"\n  live step {space}: loss {rl:.2e}  parameter gradient rel {_rel(g, rg):.2e} cos {cos_p:.5f}  x gradient cos {cos_x:.5f}")
    assert rl < 1e-2 and cos_p > 0.98 and cos_x > 0.98


def test_reset_restart_and_two_identical_runs():
    clean, wav = _clip_pair()
    op = _blind()
    y = op.forward(clean.cuda(), params=TRUE)
    wd = wav.cuda()
    start = torch.from_numpy(F.rows_phi([START] * 2)).float()
    runs = []
    for _ in range(2):
        op.reset_cache()
        out = [op.guidance(wd, LEN, y, "mel_spectrogram") for _ in range(3)]
        runs.append((out, op.phi_estimate.clone(), op.table_estimate.clone(), op._m.clone(), op._v.clone(), op.k))
    assert runs[0][5] == runs[1][5] == 3 and not torch.equal(runs[0][1].cpu(), start)
    assert _same(runs[0][1:5], runs[1][1:5])
    assert all(_same(p, q) for p, q in zip(runs[0][0], runs[1][0]))
    op.reset_cache()
    th_start = op.table_estimate.clone()
    assert torch.equal(th_start.cpu(), torch.from_numpy(F.table(SimpleNamespace(P=[D.params(knee_db=6.0, **START)] * 2, W=6.0, B=2))))
    for again in (op.reset_cache, op.restart):                     # restart: what the pipeline calls after a NaN-retry
        op.guidance(wd, LEN, y, "wav_form")
        assert op.k >= 1 and not torch.equal(op.table_estimate, th_start)
        again()
        assert op.k == 0 and torch.equal(op.phi_estimate.cpu(), start) and not op._m.any() and not op._v.any()
        assert torch.equal(_bits(op.table_estimate), _bits(th_start))
    op.apply(wd[:1], LEN)                                          # another batch: the state is made again
    assert op.phi_estimate.shape == (1, 5) and op.table_estimate.shape == (1, 8)
    three = _blind(fit=("threshold", "ratio", "makeup"))           # the times are not in fit: their bits stay
    three.forward(clean.cuda(), params=TRUE)
    three.apply(wd, LEN)
    th0, phi0 = three.table_estimate.clone(), three.phi_estimate.clone()
    for _ in range(3):
        three.guidance(wd, LEN, y, "wav_form")
    assert torch.equal(_bits(three.table_estimate[:, 3:7]), _bits(th0[:, 3:7])) and torch.equal(_bits(three.phi_estimate[:, 3:]), _bits(phi0[:, 3:]))
    assert not three._m[:, 3:].any() and not three._v[:, 3:].any() and not torch.equal(three.phi_estimate[:, :3], phi0[:, :3])


# ---- recovery -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(F.REC_FITS))
def test_estimate_recovers_known_compressor_settings(which):
    """No networks: x fixed gated noise (F.recovery_inputs), L = 6400, the true compressor -24 dB, ratio 4, knee 6, 5 / 100 ms, make-up
    +3; start -18 dB, ratio 2, 10 / 50 ms, make-up 0 (the times at the truth when only three parameters are fitted); 400 wav_form steps.
    The bounds are the issue's; the float64 restatement of this loop (F.recovery_loop_float64, asserted in
    tests/test_drc_fit_bound_host.py to stay under half of each) ends at residuals <= 1.2e-2 and |dT| <= 0.16 dB."""
    from diffmusic_amd import inverse_problem as P
    fit = F.REC_FITS[which]
    x = torch.from_numpy(F.recovery_inputs()).cuda()
    op = P.BlindDynamicRangeOperator(knee_db=F.REC_W, fit=fit, init=F.recovery_start(fit), lr=dict(zip(("threshold", "slope", "makeup", "attack", "release"), F.LR)))
    y = op.forward(x, params=F.REC_TRUE)
    ny = torch.linalg.vector_norm(y, dim=1)
    op.reset_cache()
    first, _ = op.guidance(x, F.REC_L, y, "wav_form")
    for _ in range(F.REC_STEPS - 1):
        last, _ = op.guidance(x, F.REC_L, y, "wav_form")
    assert op.k == F.REC_STEPS
    final = torch.linalg.vector_norm(op.apply(x, F.REC_L)[0] - y, dim=1) / ny
    err = np.abs(op.phi_estimate.double().cpu().numpy() - F.rows_phi([F.REC_TRUE] * 3))
    first = (first.reshape(-1) / ny).cpu().numpy()
    print(f"\n  recovery fit = {which}, seeds {F.REC_SEEDS}: residual {first} -> {final.cpu().numpy()}; |dT| {err[:, 0]}  |dk| {err[:, 1]}  "
          f"|dm| {err[:, 2]}  |d ln a| {err[:, 3:].max(1)}")
    Bd = F.REC_BOUNDS
    assert bool((first > Bd["start_residual"]).all())
    assert float(final.max()) < Bd["residual"] and err[:, 0].max() < Bd["T"] and err[:, 1].max() < Bd["k"] and err[:, 2].max() < Bd["m"]
    assert err[:, 3:].max() < Bd["ln_a"]


# ---- scheduler step and pipeline ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    from diffmusic_amd.engine import HifiGanEngine, VaeDecoderEngine
    voc, vae = HifiGanEngine(HIFI), VaeDecoderEngine(VAE)
    voc.load_state_dict(voc.synth_state_dict(seed=1))
    vae.load_state_dict(vae.synth_state_dict(seed=2))
    return voc, vae


@pytest.mark.parametrize("name,eta,rate", [("dps", 0.0, 5e-4), ("dsg", 1.0, 0.08)])
def test_scheduler_step_equals_the_fixed_parameter_operator(nets, name, eta, rate):
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    voc, vae = nets
    clean, _ = _clip_pair()
    blind = _blind()
    y = blind.forward(clean.cuda(), params=TRUE)
    known = P.DynamicRangeOperator(16000, knee_db=6.0, **START)
    start = torch.from_numpy(F.rows_phi([START] * 2)).float()
    g = torch.Generator().manual_seed(9)
    x, e, z = (torch.randn(2, 8, H, LAT_W, generator=g).cuda() for _ in range(3))
    outs = []
    for op, opk in ((blind, dict(update_drc=False)), (known, None), (blind, None)):
        s = get_scheduler(name)(operator=op, per_clip_norm=True, **SCHED)
        s.set_timesteps(200)
        noise_kw = dict(sample_noise=z) if name == "dsg" else {}
        outs.append(s.step(e, 501, x, measurement=y, vae=vae, vocoder=voc, op_kwargs=opk, eta=eta, ip_guidance_rate=rate,
                           original_waveform_length=LEN, supervised_space="mel_spectrogram", **noise_kw))
        if opk:
            assert blind.k == 0 and torch.equal(blind.phi_estimate.cpu(), start)
    assert torch.equal(_bits(outs[0].prev_sample), _bits(outs[1].prev_sample)) and torch.equal(_bits(outs[0].loss), _bits(outs[1].loss))
    assert bool(torch.isfinite(outs[0].prev_sample).all()) and not torch.equal(outs[0].prev_sample, x)
    assert torch.equal(outs[2].prev_sample, outs[1].prev_sample)
    assert blind.k == 1 and not torch.equal(blind.phi_estimate.cpu(), start)


N_CALL, SECONDS = 4, 0.4


def _pipe(op, per_clip=True):
    from diffmusic_amd.pipelines import get_pipeline
    from diffmusic_amd.schedulers import get_scheduler
    from tests.test_gpu_warm_start import HIFI as HIFI_SR, UNET
    pipe = get_pipeline("musicldm").from_pretrained("synthetic", seed=0, unet_config=UNET, vae_config=VAE, vocoder_config=HIFI_SR).to("cuda")
    pipe.scheduler = get_scheduler("dps")(operator=op, per_clip_norm=per_clip, **SCHED)
    pipe.assume_uncond_equals_cond = True
    return pipe


def _call(pipe, pe, y, n):
    return pipe(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0,
                generator=[torch.Generator().manual_seed(300 + k) for k in range(n)], output_type="pt").audios


def _inside(op):
    phi = op.phi_estimate.double().cpu().numpy()
    return bool(np.isfinite(phi).all() and (phi >= np.array(op.box_lo) - 1e-6).all() and (phi <= np.array(op.box_hi) + 1e-6).all())


def test_pipeline_call_is_finite_moves_the_estimate_repeats_and_is_the_same_in_both_bindings(monkeypatch):
    from diffmusic_amd import inverse_problem as P, ops
    clean, _ = _clip_pair()
    op = _blind(noiser=P.get_noiser("gaussian", 0.0))
    pipe = _pipe(op)
    y = op.forward(clean.cuda(), params=TRUE)
    start = torch.from_numpy(F.rows_phi([START] * 2)).float()
    pe = torch.nn.functional.normalize(torch.randn(2, 512, generator=torch.Generator().manual_seed(4)), dim=-1)
    got = []
    for torch_ops in (True, True, False):
        monkeypatch.setattr(ops, "USE_TORCH_OPS", torch_ops)
        a = _call(pipe, pe, y, 2)
        assert a.shape == (2, LEN) and bool(torch.isfinite(a).all()) and pipe.nan_restarts == 0 and op.k == N_CALL
        est = op.phi_estimate.clone()
        assert _inside(op) and not torch.equal(est.cpu(), start) and op.drc_estimate.shape == (2, 5)
        got.append((a, est, op.table_estimate.clone()))
    assert _same(got[0], got[1]), "two calls repeat"
    assert _same(got[0], got[2]), "both bindings agree"
    with pytest.raises(ValueError, match="BlindDynamicRangeOperator cannot run as clip lanes"):
        pipe(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, lanes=2)
    with pytest.raises(ValueError, match="BlindDynamicRangeOperator cannot be sharded"):
        pipe(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, shard=True)


def test_track_mode_call_with_a_batch_one_estimate():
    from diffmusic_amd import inverse_problem as P
    T, R = 11200, 1600                                        # two windows of LEN = 6400 at 0 and 4800
    lay = P.TrackLayout(T, LEN, R)
    assert lay.num_windows == 2
    inner = _blind()
    top = P.TrackOperator(inner, lay)
    pipe = _pipe(top, per_clip=False)
    clean = torch.from_numpy(D.gated_noise(np.random.default_rng(8), T)).float()[None]
    y = top.forward(clean.cuda(), params=TRUE)
    assert inner.true_params == TRUE and y.shape == (1, T)
    pe = torch.nn.functional.normalize(torch.randn(2, 512, generator=torch.Generator().manual_seed(8)), dim=-1)
    outs = []
    for _ in range(2):
        out = _call(pipe, pe, y, 2)
        assert out.shape == (1, T) and bool(torch.isfinite(out).all())
        assert inner.phi_estimate.shape == (1, 5) and inner.k == N_CALL and _inside(inner)
        outs.append((out, inner.phi_estimate.clone()))
    assert _same(outs[0], outs[1])


def test_mixture_call_with_a_batch_one_estimate():
    from diffmusic_amd import inverse_problem as P
    K = 2
    inner = _blind()
    top = P.MixtureOperator(inner, K, [1.0, 0.5])
    pipe = _pipe(top, per_clip=False)
    clean, _ = _clip_pair()
    y = top.forward(clean.cuda(), params=TRUE)
    assert inner.true_params == TRUE and y.shape == (1, LEN)
    pe = torch.nn.functional.normalize(torch.randn(K, 512, generator=torch.Generator().manual_seed(4)), dim=-1)
    outs = []
    for _ in range(2):
        out = _call(pipe, pe, y, K)
        assert out.shape == (K, LEN) and bool(torch.isfinite(out).all())
        assert inner.phi_estimate.shape == (1, 5) and inner.k == N_CALL and _inside(inner)
        outs.append((out, inner.phi_estimate.clone()))
    assert _same(outs[0], outs[1])
