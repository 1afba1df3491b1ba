"""CPU: the blind time-warp operator without a GPU (csrc/warp_fit.hip, BlindTimeWarpOperator) -- the float64 model
of tests/warp_fit_cases.py against finite differences of the loss, the transpose identity of the coarse parametrisation, the fp32
emulation of the kernel inside the element-wise bound on every case and every mutant outside it, a chain of updates that never leaves the
curve's contract, the float64 recovery loop, the constructor's and the pipelines' refusals, the helpers and the example's argument rules."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import warp_cases as W
from tests import warp_fit_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model is the gradient
@pytest.mark.parametrize("L,kind", [(1000, "walk"), (200, "small"), (65, "walk")])
def test_fine_gradient_equals_central_differences_of_the_float64_loss(L, kind):
    """dd against central differences of 0.5 ||A_d x - y||^2 in single knots, 1e-6 relative, at knot 0, an interior knot and knot H"""
    rng = np.random.default_rng(L)
    x, y = rng.standard_normal((1, L)), rng.standard_normal((1, L))
    K = F.knots(L)
    d = (W.random_walk(rng, K, 4.0, 3.3).astype(np.float64) if kind == "walk" else rng.uniform(-0.9, 0.9, K))[None] + 0.123456789

    def loss(dk):
        return 0.5 * float(((W.model(x, dk, L).y - y) ** 2).sum())
    u = W.model(x, d, L).y - y
    dd = F.fine_grad(F.model(x, u, d, L).part)[0]
    h = 1e-6
    for j in (0, (K - 1) // 2, K - 1):
        e = np.zeros_like(d)
        e[0, j] = h
        fd = (loss(d + e) - loss(d - e)) / (2 * h)
        print(f"  L={L} knot {j}: dd {dd[j]:.10g}  finite difference {fd:.10g}")
        assert abs(fd - dd[j]) <= 1e-6 * abs(dd[j]), (L, j, fd, dd[j])


@pytest.mark.parametrize("L,S", [(1, 1), (65, 2), (1000, 4), (6400, 16), (6400, 64), (70000, 32)])
def test_coarse_gradient_is_the_transpose_of_the_expansion(L, S):
    rng = np.random.default_rng(L + S)
    K, n = F.knots(L), F.coarse_knots(L, S)
    dd, e = rng.standard_normal((2, K)), rng.standard_normal((2, n))
    E = F.expand_matrix(L, S)
    from diffmusic_amd.inverse_problem import dsp
    assert n == dsp.warp_coarse_knots(L, S) and np.allclose(E.sum(1), 1.0)
    exp = dsp.warp_expand(e.astype(np.float32), L, S)
    assert exp.dtype == np.float32 and exp.shape == (2, K)
    assert np.abs(exp - e.astype(np.float32).astype(np.float64) @ E.T).max() <= 4e-7 * np.abs(e).max()       # the fp32 expansion is the model's
    assert np.array_equal(exp[:, ::S], e.astype(np.float32)[:, :exp[:, ::S].shape[1]])                  # q = 0: the coarse knot itself
    lhs, rhs = (F.coarse_grad(dd, L, S) * e).sum(1), (dd * (e @ E.T)).sum(1)
    assert np.all(np.abs(lhs - rhs) <= 1e-12 * np.abs(dd).sum(1) * np.abs(e).max()), (lhs, rhs)
    _, dc32 = F.total32(np.stack([dd[:, :-1], np.zeros((2, K - 1))], -1).astype(np.float32), L, S)       # part with b = 0: dd = (a, 0)
    ref = F.coarse_grad(np.concatenate([dd[:, :-1].astype(np.float32), np.zeros((2, 1))], 1), L, S)
    assert np.abs(dc32 - ref).max() <= 1e-5 * np.abs(dd).max() * min(2 * S, K)


# ---- the bound holds for the kernel's arithmetic and catches the mutants
@pytest.mark.parametrize("c", F.CASES, ids=lambda c: c.name)
def test_emulation_lies_within_the_bound_in_every_element(c):
    i = F.inputs(c)
    r = F.reference(c)
    part = F.emulate(i.x, i.dy, i.delay, c.L)
    assert part.shape == (c.B, c.H, 2) and part.dtype == np.float32
    ratio = F.ratio(part, r.part, r.q)
    print(f"  {c.name}: largest |emulation - model| / bound = {ratio:.4f}")
    assert ratio <= 1.0, (c.name, ratio)
    dd32, _ = F.total32(part, c.L, 4)
    assert F.ratio(dd32, F.fine_grad(r.part), F.fine_bound(r)) <= 1.0
    if c.signal == "silence" or c.dy == "zero":
        assert not part.any(), "every part is a zero"


@pytest.mark.parametrize("name", sorted(F.MUTANTS))
def test_every_mutant_leaves_the_bound(name):
    stage, cases = F.MUTANTS[name]
    worst = {n: F.run_mutant(F.CASE[n], name, stage) for n in cases}
    print(f"  {name} ({stage}): {worst}")
    assert max(worst.values()) > 1.0, (name, worst)
    assert len(F.MUTANTS) >= 8


def test_a_nan_in_one_clip_leaves_the_other_clips_rows_bit_identical():
    c = F.CASE["L1000_stride"]
    i = F.inputs(c)
    clean = F.emulate(i.x, i.dy, i.delay, c.L)
    for which in ("x", "dy"):
        x, dy = i.x.copy(), i.dy.copy()
        (x if which == "x" else dy)[1, 500] = np.nan
        part = F.emulate(x, dy, i.delay, c.L)
        assert np.array_equal(part[0].view(np.int32), clean[0].view(np.int32)) and np.array_equal(part[2].view(np.int32), clean[2].view(np.int32))
        bad = np.isnan(part[1]).any(axis=1)
        assert 1 <= bad.sum() <= 3 and np.array_equal(part[1][~bad].view(np.int32), clean[1][~bad].view(np.int32)), which
        assert which == "x" or bad[500 // 64]                       # dy[n] stays in its block; x[m] is read wherever the curve points


# ---- the update keeps the contract by construction
@pytest.mark.parametrize("S,M", [(1, 8.0), (4, 32.0), (16, 128.0), (64, 512.0), (16, 5.5)])
@pytest.mark.parametrize("anchor", ["mean", "none"])
def test_a_chain_of_updates_stays_inside_the_contract_of_the_curve(S, M, anchor):
    """From init = "zero", lr large enough to reach the clamps within a few steps, gradients whose sign alternates from coarse knot to
    coarse knot (neighbours run into opposite clamps: the steepest curve the box allows) and then flips: every curve written passes
    dsp.check_warp_curve."""
    from diffmusic_amd.inverse_problem import dsp
    L = 64 * (5 * S + 3)
    n = F.coarse_knots(L, S)
    rng = np.random.default_rng(S)
    c, m, v = np.zeros((2, n)), np.zeros((2, n)), np.zeros((2, n))
    hit = [False, False]
    for k in range(1, 41):
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 if (k // 10) % 2 == 0 else -1.0)
        dc = sign * rng.uniform(0.5, 2.0, (2, n))
        c, m, v = F.model_update(dc, c, m, v, k, lr=M / 3.0, max_delay=M, anchor=anchor)
        c32 = c.astype(np.float32)
        assert np.abs(c32).max() <= M
        fine = dsp.warp_expand(c32, L, S)
        dsp.check_warp_curve(fine, f"step {k}")
        hit[0] |= bool((c32 == M).any())
        hit[1] |= bool((c32 == -M).any())
    assert all(hit), "both clamps were reached"                   # (the clamp follows the anchor: the mean need not be zero after it)


def test_update_model_keeps_a_clip_with_a_non_finite_gradient():
    n = 7
    c0, m0, v0 = np.full((3, n), 0.5), np.full((3, n), 0.1), np.full((3, n), 0.01)
    dc = np.ones((3, n))
    dc[1, 3] = np.nan
    c, m, v = F.model_update(dc, c0, m0, v0, 2)
    assert np.array_equal(c[1], c0[1]) and np.array_equal(m[1], m0[1]) and np.array_equal(v[1], v0[1])
    assert not np.array_equal(c[0], c0[0]) and abs(c[0].mean()) < 1e-12 and np.isfinite(c).all()


def test_recovery_loop_in_float64():
    """200 wav_form steps on the fixed band-limited x from the zero curve: the estimate reaches the true coarse curve (the issue's bound for
    the device is 0.05); step 1 is still where it started."""
    errs = F.recovery_loop_float64(F.REC_STEPS, seed=0)
    print(f"  float64 recovery: step 1 {errs[0]:.3f}, step 100 {errs[99]:.2e}, step 200 {errs[-1]:.2e}")
    assert errs[0] > 0.9 and errs[-1] <= 0.05


# ---- the operator's argument rules (no GPU: the front end and the state are made on first use)
def test_constructor_refusals_by_name():
    from diffmusic_amd import constants, inverse_problem as P
    op = P.BlindTimeWarpOperator()
    assert (op.knot_stride, op.max_delay, op.lr, op.betas, op.anchor, op.k) == (16, 128.0, 0.1, (0.9, 0.999), "mean", 0)
    assert op.warp_estimate is None and op.delay_estimate is None and op.true_delay is None and op.dead_span(6400) is None
    for S in (0, 3, 128, 2.5, True, None):
        with pytest.raises(ValueError, match="knot_stride"):
            P.BlindTimeWarpOperator(knot_stride=S)
    for S, M in ((16, 128.5), (1, 9.0), (64, 4097.0), (4, 0.0), (4, -1.0), (4, float("nan"))):
        with pytest.raises(ValueError, match="max_delay"):
            P.BlindTimeWarpOperator(knot_stride=S, max_delay=M)
    P.BlindTimeWarpOperator(knot_stride=64, max_delay=512.0)
    P.BlindTimeWarpOperator(knot_stride=1, max_delay=8.0)
    with pytest.raises(ValueError, match="anchor"):
        P.BlindTimeWarpOperator(anchor="median")
    with pytest.raises(ValueError, match="init"):
        P.BlindTimeWarpOperator(init="flat")
    with pytest.raises(ValueError, match="init"):
        P.BlindTimeWarpOperator(init=np.full(8, 129.0, np.float32))
    with pytest.raises(ValueError, match="init"):
        P.BlindTimeWarpOperator(init=np.array([0.0, np.inf, 0.0], np.float32))
    with pytest.raises(ValueError, match="init"):
        P.BlindTimeWarpOperator(init=np.zeros((2, 3, 4), np.float32))
    for kw in (dict(lr=0.0), dict(lr=float("inf"))):
        with pytest.raises(ValueError, match="lr"):
            P.BlindTimeWarpOperator(**kw)
    with pytest.raises(ValueError, match="betas"):
        P.BlindTimeWarpOperator(betas=(0.9, 1.0))
    with pytest.raises(ValueError, match="adam_eps"):
        P.BlindTimeWarpOperator(adam_eps=-1.0)
    with pytest.raises(ValueError, match="sample_rate"):
        P.BlindTimeWarpOperator(sample_rate=0)
    init = np.array([[1.0, 2.0, 3.0], [-120.0, 0.0, 126.0]], np.float32)
    assert torch.equal(P.BlindTimeWarpOperator(init=init)._start, torch.tensor([[-1.0, 0.0, 1.0], [-122.0, -2.0, 124.0]]))
    assert torch.equal(P.BlindTimeWarpOperator(init=init, anchor="none")._start, torch.from_numpy(init))
    with pytest.raises(ValueError, match="dsp.wow_curve"):
        op.forward(torch.zeros(2, 6400))
    with pytest.raises(ValueError, match=r"warp_knots\(6400\)"):
        op.forward(torch.zeros(2, 6400), delay=np.zeros(50, np.float32))
    with pytest.raises(ValueError, match="limit is 16"):
        op.forward(torch.zeros(2, 6400), delay=np.where(np.arange(101) % 2 == 0, 9.0, -9.0).astype(np.float32))
    with pytest.raises(ValueError, match="3, 101"):
        op.forward(torch.zeros(2, 6400), delay=np.zeros((3, 101), np.float32))
    wrong = P.BlindTimeWarpOperator(init=np.zeros(5, np.float32))
    with pytest.raises(ValueError, match=r"warp_coarse_knots\(6400, 16\) = 8"):
        wrong.apply(torch.zeros(2, 6400), 6400)
    with pytest.raises((RuntimeError, AssertionError)):
        op.forward(torch.zeros(2, 6400), delay=np.zeros(101, np.float32))                # no CPU fallback
    assert torch.equal(op.true_delay, torch.zeros(2, 101))                              # the curve was kept all the same
    assert constants.MUSIC_BLIND_WOW_FLUTTER == "music_blind_wow_flutter"


def test_helpers():
    from diffmusic_amd.inverse_problem import dsp
    assert [dsp.warp_coarse_knots(6400, S) for S in (1, 2, 4, 8, 16, 32, 64)] == [101, 51, 26, 14, 8, 5, 3]
    assert dsp.warp_coarse_knots(1, 64) == 2 and dsp.warp_coarse_knots(64 * 64 + 1, 64) == 3
    for bad in (0, 3, 128, True):
        with pytest.raises(ValueError, match="knot_stride"):
            dsp.warp_coarse_knots(6400, bad)
    with pytest.raises(ValueError, match="warp_coarse_knots"):
        dsp.warp_expand(np.zeros(9, np.float32), 6400, 16)
    fine = dsp.warp_expand(np.array([0.0, 16.0, -16.0], np.float32), 64 * 5, 4)
    assert fine.tolist() == [0.0, 4.0, 8.0, 12.0, 16.0, 8.0]


def test_pipeline_refuses_lanes_and_shards():
    from types import SimpleNamespace
    from diffmusic_amd.pipelines.pipeline_musicldm import MusicLDMPipeline
    from diffmusic_amd import inverse_problem as P

    def check(op, **kw):
        pipe = SimpleNamespace(scheduler=SimpleNamespace(operator=op), lanes=1)
        return MusicLDMPipeline._check_positional_state(pipe, kw.get("shard", False), kw.get("group"), kw.get("lanes"))
    op = P.BlindTimeWarpOperator()
    track = P.TrackOperator(op, P.TrackLayout(11200, 6400, 1600))
    for o in (op, track, P.MixtureOperator(op, 2), P.MixtureOperator(track, 2)):
        check(o)
        with pytest.raises(ValueError, match="BlindTimeWarpOperator cannot run as clip lanes"):
            check(o, lanes=2)
        for kw in (dict(shard=True), dict(group=object())):
            with pytest.raises(ValueError, match="BlindTimeWarpOperator cannot be sharded"):
                check(o, **kw)


def test_abi_surface_lists_the_new_entry_points():
    from diffmusic_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "diffmusic_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    torch_ops = open(os.path.join(ROOT, "diffmusic_amd", "csrc_torch", "torch_ops.cpp")).read()
    for name in ("dmx_warp_wgrad", "dmx_warp_update"):
        assert name in _lib._SIGS and name in _lib.ADDED_IN_V4
        assert re.search(rf"\b{name}\s*\(", header), name
        assert f"#pragma weak {name}\n" in torch_ops, name
    assert _lib.ABI_VERSION == 4 and "#define DMX_ABI_VERSION 4 " in header
    assert "warp_wgrad" in ops.OP_NAMES and "warp_update" in ops.OP_NAMES
    assert "warp_wgrad(Tensor dy, Tensor x, Tensor delay, int length) -> Tensor" in torch_ops
    with pytest.raises((RuntimeError, AssertionError)):
        ops.ctypes_hip.warp_wgrad(torch.zeros(1, 300), torch.zeros(1, 300), torch.zeros(6), 300)        # no CPU fallback
    warp = open(os.path.join(ROOT, "diffmusic_amd", "csrc", "warp.hip")).read()
    fit = open(os.path.join(ROOT, "diffmusic_amd", "csrc", "warp_fit.hip")).read()
    assert '#include "warp_common.h"' in warp and '#include "warp_common.h"' in fit and "float warp_delta(" not in warp + fit


# ---- examples/run_inverse_problem.py
def _example():
    spec = importlib.util.spec_from_file_location("run_inverse_problem", os.path.join(ROOT, "examples", "run_inverse_problem.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_argument_rules():
    from diffmusic_amd.config import compose
    from diffmusic_amd import constants, inverse_problem as P
    mod = _example()
    assert mod.BLIND_WOW == constants.MUSIC_BLIND_WOW_FLUTTER and mod.BLIND_WOW in mod.TASKS
    t = ("-t", mod.BLIND_WOW)

    def fit(*argv, cfg=None):
        return mod.blind_warp_params(mod.parse_args(list(argv)), cfg)

    def true(*argv, cfg=None):
        return mod.warp_params(mod.parse_args(list(argv)), cfg)
    assert fit(*t) == dict(knot_stride=16, max_delay=128.0, lr=0.1)
    assert fit(*t, "--warp_knot_stride", "4", "--warp_max_delay", "32", "--warp_lr", "0.05") == dict(knot_stride=4, max_delay=32.0, lr=0.05)
    for bad in (("--warp_knot_stride", "3"), ("--warp_knot_stride", "128"), ("--warp_max_delay", "129"), ("--warp_knot_stride", "4"),
                ("--warp_lr", "0"), ("--warp_lr", "nan"), ("--warp_max_delay", "-1")):
        with pytest.raises(SystemExit):
            fit(*t, *bad)                                            # stride 4 alone leaves max_delay = 128 > 32
    for other in ("music_inpainting", "music_wow_flutter"):
        assert fit("-t", other) is None
        for flag in ("--warp_knot_stride", "--warp_max_delay", "--warp_lr"):
            with pytest.raises(SystemExit, match="music_blind_wow_flutter"):
                fit("-t", other, flag, "4")
    assert true(*t) == dict(components=(), speed_percent=0.0)        # --wow / --speed_pct describe the TRUE curve of this task too
    assert true(*t, "--wow", "0.5,1", "--speed_pct", "-0.5") == dict(components=((0.5, 1.0),), speed_percent=-0.5)
    with pytest.raises(SystemExit, match="music_blind_wow_flutter"):
        true("-t", "music_inpainting", "--wow", "1,1")
    args = mod.parse_args([*t, "--track_overlap_s", "1.28"])          # track mode is allowed
    assert args.track_overlap_s == 1.28 and mod.spectral_boxes(args) is None and mod.compressor_params(args) is None
    cfg = compose("dps", overrides=["data=moises", "model=musicldm", f"inverse_problem={mod.BLIND_WOW}"])
    assert cfg.inverse_problem.noise.name == "gaussian" and float(cfg.inverse_problem.noise.sigma) == 0.0
    assert fit(*t, cfg=cfg) == dict(knot_stride=16, max_delay=128.0, lr=0.1)
    assert fit(*t, "--warp_lr", "0.3", cfg=cfg) == dict(knot_stride=16, max_delay=128.0, lr=0.3)      # a flag wins, the rest stays
    warp = true(*t, cfg=cfg)
    assert warp == dict(components=((0.5, 1.0, 0.0), (9.0, 0.2, 0.0)), speed_percent=0.0)
    op, scale = mod.build_operator(mod.BLIND_WOW, cfg, "box", warp=warp, blind_warp=fit(*t, cfg=cfg))
    length = int(cfg.model.pipe.audio_length_in_s * cfg.data.sample_rate)
    assert isinstance(op, P.BlindTimeWarpOperator) and scale == 1 and op.sample_rate == cfg.data.sample_rate and op.noiser is not None
    assert (op.knot_stride, op.max_delay, op.lr, op.anchor) == (16, 128.0, 0.1, "mean")
    assert np.array_equal(op.true_delay.numpy()[0], P.wow_curve(length, cfg.data.sample_rate, **warp))
    track, _ = mod.build_operator(mod.BLIND_WOW, cfg, "box", audio_length_in_s=P.seconds_for_samples(3 * length - 7, cfg.data.sample_rate),
                                  warp=warp, blind_warp=fit(*t, cfg=cfg))
    assert track.true_delay.shape == (1, P.warp_knots(3 * length - 7))       # the true curve is built for the track's length
    with pytest.raises(ValueError):
        mod.build_operator(mod.BLIND_WOW, cfg, "box", warp=warp)
