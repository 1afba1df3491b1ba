"""CPU: the blind equalisation without a GPU (csrc/tf_eq.hip, BlindEqualizationOperator) -- the fp32 emulation of the
curve gradient lies inside the element-wise bound for every case and every mutant leaves it, the adjoint identity in g on the float64
model, the update against hand-computed first steps, the operator's construction and refusals, the curve helpers, the ABI surface, the
example's argument rules, and the recovery loop of tests/test_gpu_blind_eq.py restated in float64 on that test's own inputs."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import tf_eq_cases as EQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- bound, emulation, mutants
@pytest.mark.parametrize("c", EQ.CASES, ids=lambda c: c.name)
def test_emulation_lies_within_the_bound(c):
    r = EQ.run_case(c)
    print(f"{c.name}: emulation / bound {r:.3f}")
    assert r <= 1.0, (c.name, c.why, r)


def test_case_table_covers_the_segment_edges():
    assert EQ.SEG == 16
    assert {c.L for c in EQ.CASES} >= {300, 1024, 1025, 3328, 3329, 4999, 6400, 9000} and all(c.B <= 3 for c in EQ.CASES)
    assert (EQ.CASE["L3328"].T, EQ.CASE["L3328"].S) == (16, 1) and (EQ.CASE["L3329"].T, EQ.CASE["L3329"].S) == (17, 2)
    assert (EQ.CASE["L9000"].T, EQ.CASE["L9000"].S) == (39, 3) and EQ.CASE["L6400_stride"].stride_x > 6400 < EQ.CASE["L6400_stride"].stride_dy


def test_zero_cotangent_gives_plus_zero_and_a_zero_bound():
    c = EQ.CASE["L4999_dy_zero"]
    r, q = EQ.reference(c)
    assert not r.dg.any() and not q.any()
    part = EQ.emulate(EQ.inputs(c).x, EQ.inputs(c).dy, c.L)
    assert part.shape == (3, 2, 513) and not part.any() and not np.signbit(part).any()


@pytest.mark.parametrize("name", sorted(EQ.MUTANTS))
def test_every_mutant_leaves_the_bound(name):
    where, cases = EQ.MUTANTS[name]
    worst = {n: EQ.run_case(EQ.CASE[n], name, where) for n in cases}
    print(f"{name} ({where}): " + "  ".join(f"{n} {v:.3g}" for n, v in worst.items()))
    assert max(worst.values()) > 1.0, (name, worst)


def test_the_gradient_is_the_adjoint_in_the_curve():
    """<dy, A_g x> = sum_k g_k dg_k on the float64 model: A is linear in g."""
    for name in ("L300", "L4999", "L9000"):
        c = EQ.CASE[name]
        i = EQ.inputs(c)
        g = np.random.default_rng(len(name)).uniform(0.0, 1.5, (c.B, 513))
        lhs = (i.dy.astype(np.float64) * EQ.model_apply(i.x, g, c.L)).sum(1)
        rhs = (g * EQ.reference(c)[0].dg).sum(1)
        assert np.abs(lhs - rhs).max() <= 1e-12 * np.abs(lhs).max(), (name, lhs, rhs)
    x = EQ.inputs(EQ.CASE["L1025"]).x
    assert np.abs(EQ.model_apply(x, np.ones(513), 1025) - x).max() <= 1e-13           # A_1 = I


# ---- the update
def test_model_update_first_steps_by_hand():
    lr, eps = 0.05, 1e-8
    dg = np.zeros((4, 513))
    dg[0, :] = 0.5                                            # k = 1: m' / (1 - b1) = dg, v' / (1 - b2) = dg^2: a step of lr sign(dg)
    dg[0, 7] = -0.25
    dg[1, :] = 1.0
    dg[2, :] = 1.0
    dg[2, 3] = math.nan
    g0 = np.ones((4, 513))
    g0[1, :] = 0.04                                           # driven below zero everywhere: the clamp, then a zero peak
    z = np.zeros((4, 513))
    g, m, v = EQ.model_update(dg, g0, z, z, 1, lr=lr, eps=eps, peak=False)
    assert np.allclose(np.delete(g[0], 7), 1 - lr, atol=1e-8) and abs(g[0, 7] - (1 + lr)) <= 1e-8      # eps / |dg| <= 4e-8 of lr
    assert np.allclose(m[0], 0.1 * dg[0]) and np.allclose(v[0], 0.001 * dg[0] ** 2)
    assert not g[1].any() and not np.signbit(g[1]).any() and abs(m[1, 0] - 0.1) <= 1e-15       # "none": the clamp alone is no reason to keep
    assert (g[2] == 1).all() and not m[2].any() and not v[2].any()                # a NaN in dg: the clip keeps (g, m, v)
    assert (g[3] == 1).all() and not m[3].any()                                   # dg = 0: step 0 / (0 + eps) = 0
    g, m, v = EQ.model_update(dg, g0, z, z, 1, lr=lr, eps=eps, peak=True)
    assert abs(g[0, 7] - 1.0) <= 1e-12 and np.allclose(np.delete(g[0], 7), (1 - lr) / (1 + lr), atol=1e-8)
    assert (g[1] == 0.04).all() and not m[1].any() and not v[1].any()             # max g~ == 0 under "peak": kept
    assert (g[2] == 1).all() and (g[3] == 1).all()
    # second step from the first, by hand: m2 = b1 m1 + (1 - b1) d, bias corrections 1 - b1^2, 1 - b2^2
    d = np.full((1, 513), 0.5)
    g1, m1, v1 = EQ.model_update(d, np.ones((1, 513)), z[:1], z[:1], 1, lr=lr, eps=eps, peak=False)
    g2, m2, v2 = EQ.model_update(-d, g1, m1, v1, 2, lr=lr, eps=eps, peak=False)
    m_hand, v_hand = 0.9 * 0.05 - 0.1 * 0.5, 0.999 * 0.00025 + 0.001 * 0.25
    step = lr * (m_hand / (1 - 0.81)) / (math.sqrt(v_hand / (1 - 0.999 ** 2)) + eps)
    assert abs(m2[0, 0] - m_hand) <= 1e-15 and abs(v2[0, 0] - v_hand) <= 1e-15 and abs(g2[0, 0] - (g1[0, 0] - step)) <= 1e-12


# ---- the operator without a GPU
def _op(**kw):
    from diffmusic_amd.inverse_problem import BlindEqualizationOperator
    return BlindEqualizationOperator(**kw)


def test_constructor_and_refusals_need_no_gpu():
    op = _op()
    assert op.eq_estimate is None and op.true_curve is None and op.k == 0 and op.dead_span(6400) is None
    assert (op.lr, op.betas, op.adam_eps, op.normalize) == (0.05, (0.9, 0.999), 1e-8, "peak")
    assert tuple(op._start.shape) == (1, 513) and bool((op._start == 1).all())
    for lr in (0, -1.0, math.nan, math.inf, "x"):
        with pytest.raises(ValueError, match="lr"):
            _op(lr=lr)
    for betas in ((0.9,), (0.9, 1.0), (-0.1, 0.5), (0.9, 0.999, 0.5)):
        with pytest.raises(ValueError, match="betas"):
            _op(betas=betas)
    with pytest.raises(ValueError, match="adam_eps"):
        _op(adam_eps=-1e-8)
    with pytest.raises(ValueError, match="normalize"):
        _op(normalize="l2")
    for init in ("impulse", torch.ones(512), torch.ones(2, 2, 513), torch.zeros(0, 513)):
        with pytest.raises(ValueError, match="init"):
            _op(init=init)
    bad = torch.ones(513)
    for v in (math.nan, math.inf, -0.5):
        b = bad.clone()
        b[5] = v
        with pytest.raises(ValueError, match="init"):
            _op(init=b)
    with pytest.raises(ValueError, match="peak"):
        _op(init=torch.zeros(513))
    assert not _op(init=torch.zeros(513), normalize="none")._start.any()          # no peak needed without the normalisation
    rows = torch.tensor([[2.0] * 513, [0.5] * 513])
    rows[1, 10] = 4.0
    op = _op(init=rows)
    assert tuple(op._start.shape) == (2, 513) and bool((op._start.amax(dim=1) == 1).all()) and float(op._start[1, 0]) == 0.125
    assert torch.equal(_op(init=rows, normalize="none")._start, rows)
    assert _op(betas=(0.0, 0.0)).betas == (0.0, 0.0)


def test_forward_needs_a_curve_and_curves_are_checked_by_name():
    op = _op()
    x = torch.zeros(2, 6400)
    with pytest.raises(ValueError, match="true curve"):
        op.forward(x)
    with pytest.raises(ValueError, match="513"):
        op.forward(x, curve=torch.ones(512))
    with pytest.raises(ValueError, match="3 curve"):
        op.forward(x, curve=torch.ones(3, 513))
    with pytest.raises(ValueError, match="3 curve"):
        op.apply(x, 6400, curve=torch.ones(3, 513))


def test_pipeline_refuses_lanes_and_shards():
    from diffmusic_amd.pipelines.pipeline_musicldm import MusicLDMPipeline
    from diffmusic_amd import inverse_problem as P
    from types import SimpleNamespace

    def check(op, **kw):
        pipe = SimpleNamespace(scheduler=SimpleNamespace(operator=op), lanes=1)
        return MusicLDMPipeline._check_positional_state(pipe, kw.get("shard", False), kw.get("group"), kw.get("lanes"))
    op = _op()
    track = P.TrackOperator(op, P.TrackLayout(11200, 6400, 1600))
    for o in (op, track, P.MixtureOperator(op, 2), P.MixtureOperator(track, 2)):
        check(o)
        with pytest.raises(ValueError, match="BlindEqualizationOperator cannot run as clip lanes"):
            check(o, lanes=2)
        with pytest.raises(ValueError, match="BlindEqualizationOperator cannot be sharded"):
            check(o, shard=True)


# ---- dsp helpers
def test_curve_helpers():
    from diffmusic_amd.inverse_problem import eq_curve, lowpass_curve
    sr = 16000
    lp = lowpass_curve(sr, 2000.0, 4)
    assert lp.shape == (513,) and lp.dtype == np.float32 and lp[0] == 1.0
    assert abs(lp[128] - 1 / math.sqrt(2)) <= 1e-7                               # bin 128 = 2000 Hz: -3 dB
    assert abs(lp[512] - 1 / math.sqrt(1 + 4.0 ** 8)) <= 1e-9 and (np.diff(lp) <= 0).all()
    assert abs(lowpass_curve(sr, 2000.0, 1)[128] - 1 / math.sqrt(2)) <= 1e-7 and lowpass_curve(sr, 2000.0, 1)[512] > lp[512]
    for bad in ((0.0, 4), (-1.0, 4), (math.nan, 4), (1000.0, 0)):
        with pytest.raises(ValueError):
            lowpass_curve(sr, *bad)
    pts = [(125.0, 0.0), (1000.0, -6.0), (4000.0, -18.0)]                        # bins 8, 64, 256
    eq = eq_curve(sr, pts)
    assert eq.shape == (513,) and eq.dtype == np.float32
    for k, db in ((8, 0.0), (64, -6.0), (256, -18.0)):
        assert abs(eq[k] - 10 ** (db / 20)) <= 1e-6
    assert eq[0] == 1.0 and (eq[:9] == 1.0).all() and abs(eq[512] - 10 ** (-18 / 20)) <= 1e-6 and (eq[256:] == eq[256]).all()
    assert abs(eq[32] - 10 ** (-4.0 / 20)) <= 1e-6                              # 500 Hz: two of three octaves from 125 to 1000 Hz
    assert (eq_curve(sr, [(1000.0, 6.0)]) == np.float32(10 ** 0.3)).all()
    for bad in ([], [(0.0, 1.0)], [(100.0, math.nan)], [(200.0, 0.0), (100.0, 0.0)], [(100.0, 0.0), (100.0, 1.0)]):
        with pytest.raises(ValueError):
            eq_curve(sr, bad)


# ---- ABI surface
NEW = ("dmx_audio_tf_curve", "dmx_audio_tf_wgrad_segments", "dmx_audio_tf_wgrad", "dmx_audio_eq_update")


def test_abi_surface_lists_the_new_entry_points():
    from diffmusic_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "diffmusic_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    torch_ops = open(os.path.join(ROOT, "diffmusic_amd", "csrc_torch", "torch_ops.cpp")).read()
    for name in NEW:
        assert name in _lib._SIGS and name in _lib.ADDED_IN_V4
        assert re.search(rf"\b{name}\s*\(", header), name
        assert f"#pragma weak {name}\n" in torch_ops, name
    assert _lib.ABI_VERSION == 4 and "#define DMX_ABI_VERSION 4 " in header
    for op in ("tf_curve", "tf_wgrad", "eq_update"):
        assert op in ops.OP_NAMES
    with pytest.raises((RuntimeError, AssertionError)):
        ops.ctypes_hip.tf_curve(0, torch.zeros(1, 300), torch.ones(513), 300, 300)          # no CPU fallback
    with pytest.raises((RuntimeError, AssertionError)):
        ops.ctypes_hip.tf_wgrad(0, torch.zeros(1, 300), torch.zeros(1, 300), 300)


def test_the_update_kernels_share_one_adam_step():
    """ir_update keeps its arithmetic: both update kernels take the step from csrc/adam_step.h and neither restates it."""
    csrc = os.path.join(ROOT, "diffmusic_amd", "csrc")
    for name in ("fir_blind.hip", "tf_eq.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "adam_step.h"' in src and "adam_tap(" in src and "sqrtf(vn" not in src, name
    assert "contract(off)" in open(os.path.join(csrc, "adam_step.h")).read()


# ---- examples/run_inverse_problem.py
def _example():
    spec = importlib.util.spec_from_file_location("run_inverse_problem", os.path.join(ROOT, "examples", "run_inverse_problem.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_argument_rules():
    from diffmusic_amd import inverse_problem as P
    mod = _example()
    assert "music_blind_equalization" in mod.TASKS

    def curve(*argv, cfg=None):
        return mod.equalization_curve(mod.parse_args(list(argv)), cfg)
    t = ("-t", "music_blind_equalization")
    assert np.array_equal(curve(*t, "--eq_lowpass", "3000"), P.lowpass_curve(16000, 3000.0, 4))
    assert np.array_equal(curve(*t, "--eq_lowpass", "3000,2"), P.lowpass_curve(16000, 3000.0, 2))
    assert np.array_equal(curve(*t, "--eq_points", "100,0;1000,-6"), P.eq_curve(16000, [(100.0, 0.0), (1000.0, -6.0)]))
    for bad in (("--eq_lowpass", "3000", "--eq_points", "100,0"), ("--eq_lowpass", "0"), ("--eq_lowpass", "a"), ("--eq_lowpass", "3000,1.5"),
                ("--eq_lowpass", "3000,0"), ("--eq_lowpass", "3000,4,1"), ("--eq_lowpass", ""), ("--eq_points", "100"), ("--eq_points", "100,0,1"),
                ("--eq_points", "0,1"), ("--eq_points", "100,"), ("--eq_points", "200,0;100,0"), ("--eq_points", "100,inf"), ()):
        with pytest.raises(SystemExit):
            curve(*t, *bad)
    with pytest.raises(SystemExit, match="one of them"):
        curve(*t, "--eq_lowpass", "3000", "--eq_points", "100,0")
    for other in ("music_inpainting", "music_spectral_inpainting"):
        assert curve("-t", other) is None
        with pytest.raises(SystemExit, match="music_blind_equalization"):
            curve("-t", other, "--eq_lowpass", "3000")
        with pytest.raises(SystemExit, match="music_blind_equalization"):
            curve("-t", other, "--eq_points", "100,0")
    args = mod.parse_args([*t, "--track_overlap_s", "1.28"])                    # track mode is allowed
    assert args.track_overlap_s == 1.28 and mod.spectral_boxes(args) is None and mod.separation_stems(args) is None


def test_example_takes_its_curve_from_the_config_and_builds_the_operator():
    from diffmusic_amd.config import compose
    from diffmusic_amd import constants, inverse_problem as P
    mod = _example()
    assert constants.MUSIC_BLIND_EQUALIZATION == mod.BLIND_EQ == "music_blind_equalization"
    cfg = compose("dps", overrides=["data=moises", "model=musicldm", f"inverse_problem={mod.BLIND_EQ}"])
    assert cfg.inverse_problem.noise.name == "gaussian" and float(cfg.inverse_problem.noise.sigma) == 0.0
    true = mod.equalization_curve(mod.parse_args(["-t", mod.BLIND_EQ]), cfg)
    pts = [tuple(p) for p in cfg.inverse_problem.points]
    assert len(pts) >= 2 and np.array_equal(true, P.eq_curve(cfg.data.sample_rate, pts))
    op, scale = mod.build_operator(mod.BLIND_EQ, cfg, "box", eq_true=true)
    assert isinstance(op, P.BlindEqualizationOperator) and scale == 1 and op.lr == 0.05 and op.normalize == "peak"
    assert op.betas == (0.9, 0.999) and op.adam_eps == 1e-8 and torch.equal(op.true_curve, torch.from_numpy(true)[None])
    flag = mod.equalization_curve(mod.parse_args(["-t", mod.BLIND_EQ, "--eq_lowpass", "2000"]), cfg)      # flags win
    assert np.array_equal(flag, P.lowpass_curve(cfg.data.sample_rate, 2000.0, 4))
    with pytest.raises(ValueError):
        mod.build_operator(mod.BLIND_EQ, cfg, "box")


# ---- recovery, restated in float64 on the GPU test's own inputs
def test_recovery_loop_in_float64():
    """The loop of test_gpu_blind_eq.py::test_estimate_recovers_a_known_curve: from >= 0.9 it must stay <= 0.05 over steps 150 .. 200, so
    that the GPU test's 0.1 has a factor two in hand over everything the reference shows near the end."""
    x, true = EQ.recovery_inputs()
    assert x.shape == (2, 6400) and true.max() == 1.0 and not true[300:].any() and (true[:300] > 0).all()
    err = EQ.recovery_loop(x, true, 6400, steps=200)
    print(f"float64 recovery: start {err[0].tolist()}, worst of steps 150 .. 200 {err[150:].max(0).tolist()}, end {err[-1].tolist()}")
    assert err.shape == (201, 2) and (err[0] >= 0.9).all() and (err[150:] <= 0.05).all()
