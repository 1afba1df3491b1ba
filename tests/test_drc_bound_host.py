"""CPU: the dynamic-range compressor's float64 model, bound, emulation and mutants (tests/drc_cases.py) hold together, the transpose is the
transpose of the Jacobian, the host helpers, the operator's refusals, the ABI surface and the example's argument rules.  No GPU."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import drc_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the emulation against the model, element by element
@pytest.mark.parametrize("c", D.CASES, ids=lambda c: c.name)
def test_emulation_lies_within_the_bound(c):
    i = D.inputs(c)
    r, q, rb, qdx = D.reference(c)
    e = D.emulate(i.x, c.L, c.P)
    got = {"p": D.ratio(e.p, r.p, q.p), "s": D.ratio(e.s, r.s, q.s), "G": D.ratio(e.G, r.G, q.G), "y": D.ratio(e.y, r.y, q.y)}
    assert D.tape_differences_allowed(e.tape, r, q), "a tape bit differs where the model is not ambiguous"
    got["dx"] = D.judge_bwd(c, D.emulate_bwd(i.x, i.dy, c.L, c.P, e), e.tape)
    print(f"{c.name}: emulation / bound " + " ".join(f"{k} {v:.3f}" for k, v in got.items()))
    assert all(v <= 1.0 for v in got.values()), (c.name, got)


@pytest.mark.parametrize("c", D.CASES, ids=lambda c: c.name)
def test_ambiguous_blocks_stay_under_the_cap(c):
    """from the float64 model alone: at most 1 % of a case's blocks, none where H < 100"""
    _, q, _, _ = D.reference(c)
    share = D.ambiguous_share(q)
    print(f"{c.name}: H = {c.H}, ambiguous blocks {int((q.amb_rg | q.amb_att).sum())} of {c.B * c.H}")
    assert share <= D.AMBIG_CAP and (c.H >= 100 or share == 0.0), (c.name, share)


def test_case_table_covers_the_listed_shapes():
    assert {c.L for c in D.CASES} >= {1, 63, 64, 65, 1000, 6400, 20037, 70000} and all(c.B == 3 for c in D.CASES)
    assert D.CASE["L70000"].H == 1094 and D.CASE["L1000"].L - 15 * 64 == 40
    s = D.CASE["L20037_stride"]
    assert s.off % 4 != 0 and s.stride > s.full > s.L
    assert any(c.full > c.L for c in D.CASES) and {c.P.W for c in D.CASES} >= {0.0, 6.0}
    assert D.PARAMS["limiter"].k == 1.0 and D.PARAMS["fastrel"].aA < D.PARAMS["fastrel"].aR and D.PARAMS["base"].aA > D.PARAMS["base"].aR
    assert D.PARAMS["makeup"].makeup != 0.0
    for c in D.CASES:                                              # gated cases spend a real share of their blocks on either side of the gates
        if c.signal == "gated" and c.H >= 16:
            r = D.reference(c)[0]
            assert 0.2 < float((r.rg == 2).mean()) < 0.8 and 0.02 < float(r.att.mean()) < 0.98, c.name
            assert float(r.s.max()) > 8.0, c.name                  # several dB of gain reduction


def test_a_quiet_clip_is_scaled_by_the_makeup_and_silence_stays_silent():
    c = D.CASE["L6400_quiet"]
    i, (r, q, rb, qdx) = D.inputs(c), D.reference(c)
    assert not r.tape.any() and not r.s.any() and not q.s.any() and not (q.amb_rg | q.amb_att).any()
    mk = 10.0 ** (c.P.makeup / 20.0)
    assert np.allclose(r.y, mk * i.x.astype(np.float64), rtol=1e-15, atol=0) and np.allclose(rb.dx, mk * i.dy.astype(np.float64), rtol=1e-15, atol=0)
    e = D.emulate(i.x, c.L, c.P)
    assert not e.tape.any() and not e.s.any() and np.all(e.G == e.G[0, 0])
    c = D.CASE["L6400_silence"]
    r, q, rb, qdx = D.reference(c)
    assert not r.y.any() and not q.y.any() and not r.tape.any() and np.array_equal(rb.dx, D.inputs(c).dy.astype(np.float64))


# ---- mutants
@pytest.mark.parametrize("name", sorted(D.MUTANTS))
def test_every_mutant_leaves_the_bound(name):
    stage, cases = D.MUTANTS[name]
    worst = {n: D.run_mutant(D.CASE[n], name, stage) for n in cases}
    print(f"{name}: mutant / bound {worst}")
    assert max(worst.values()) > 1.0, (name, worst)


def test_the_mutant_list_is_the_issues():
    assert len(D.MUTANTS) == 9 and {s for s, _ in D.MUTANTS.values()} == {"fwd", "bwd"}
    assert all(n in D.CASE for _, names in D.MUTANTS.values() for n in names)


# ---- the transpose is the transpose of the Jacobian
@pytest.mark.parametrize("name", ["L1000", "L1000_hard", "L6400_fastrel", "L6400_limiter", "L20037_stride"])
def test_transpose_matches_a_central_difference(name):
    """<dy, J v> from a float64 central difference of the model = <J^T dy, v> to 1e-6 relative; the step keeps every gate (asserted)."""
    c = D.CASE[name]
    i, (r, q, rb, _) = D.inputs(c), D.reference(c)
    x, dy = i.x.astype(np.float64), i.dy.astype(np.float64)
    v = np.random.default_rng(5).standard_normal(x.shape)
    h = 1e-6
    up, dn = D.model(x + h * v, c.L, c.P), D.model(x - h * v, c.L, c.P)
    assert np.array_equal(up.tape, r.tape) and np.array_equal(dn.tape, r.tape), "the step crossed a gate"
    for b in range(c.B):
        lhs = float(dy[b] @ ((up.y[b] - dn.y[b]) / (2 * h)))
        rhs = float(rb.dx[b] @ v[b])
        print(f"{name}[{b}]: <dy, J v> = {lhs:.12g}, <J^T dy, v> = {rhs:.12g}")
        assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs)), (name, b, lhs, rhs)
    side = np.abs(rb.side).sum() / np.abs(rb.dx).sum()
    assert side > 1e-3, "the sidechain term takes part"


# ---- host helpers
def test_helpers():
    from diffmusic_amd.inverse_problem import drc_coeffs, drc_static_curve
    aA, aR = drc_coeffs(16000, 5.0, 100.0)
    assert aA.dtype == np.float32 and aR.dtype == np.float32
    assert aA == np.float32(1.0 - math.exp(-64 / 80.0)) and aR == np.float32(1.0 - math.exp(-64 / 1600.0))
    assert drc_coeffs(48000, 5.0, 100.0)[0] < aA
    for bad in ((0, 5, 100), (16000, 0, 100), (16000, 5, -1), (16000, math.inf, 100), (16000, 5, math.nan)):
        with pytest.raises(ValueError):
            drc_coeffs(*bad)
    with pytest.raises(ValueError, match="attack_ms"):
        drc_coeffs(16000, 0, 100)
    with pytest.raises(ValueError, match="release_ms"):
        drc_coeffs(16000, 5, 0)
    lv = np.array([-60.0, -27.0, -24.0, -21.0, -12.0, 0.0])
    c = drc_static_curve(lv, -24.0, 4.0, 6.0)
    assert np.allclose(c, [0.0, 0.0, 0.75 * 9 / 12, 0.75 * 3, 0.75 * 12, 0.75 * 24], rtol=1e-15)
    assert np.allclose(drc_static_curve(lv, -24.0, math.inf, 0.0), np.maximum(lv + 24.0, 0.0))
    assert not drc_static_curve(lv, -24.0, 1.0, 6.0).any()
    grid = np.linspace(-40.0, 0.0, 4001)
    assert np.abs(np.diff(drc_static_curve(grid, -24.0, 4.0, 6.0))).max() <= 0.75 * 0.01 * (1 + 1e-9)      # continuous, slope <= k
    for c in (D.CASE["L6400"], D.CASE["L6400_hard"], D.CASE["L6400_limiter"]):
        r = D.reference(c)[0]
        ratio = math.inf if c.P.k == 1.0 else 1.0 / (1.0 - c.P.k)
        assert np.allclose(drc_static_curve(r.l, c.P.T, ratio, c.P.W), r.c, rtol=1e-12, atol=1e-12)
    for bad in ((0.5, 6.0), (math.nan, 6.0), (4.0, -1.0), (4.0, math.inf)):
        with pytest.raises(ValueError):
            drc_static_curve(lv, -24.0, *bad)


# ---- the operator, without a GPU
def test_constructor_and_refusals_need_no_gpu():
    from diffmusic_amd import constants, inverse_problem as P
    op = P.DynamicRangeOperator()
    assert (op.sample_rate, op.threshold_db, op.ratio, op.knee_db, op.attack_ms, op.release_ms, op.makeup_db) == (16000, -24.0, 4.0, 6.0, 5.0, 100.0, 0.0)
    assert op.noiser is None and op.dead_span(6400) is None and op._on_load(None, 6400) is None and op._frontend is None
    assert op.params == D.PARAMS["base"].args and isinstance(op, P.BaseOperator)
    lim = P.DynamicRangeOperator(ratio=math.inf, knee_db=0, makeup_db=7.5, noiser=P.GaussianNoise(0.0))
    assert lim.slope == 1.0 and lim.knee_db == 0.0 and lim.params[5] == 7.5
    assert P.DynamicRangeOperator(ratio=1.0).slope == 0.0
    assert all(v == float(np.float32(v)) for v in P.DynamicRangeOperator(threshold_db=-23.3, ratio=3.0, makeup_db=0.1).params)
    for name, bad in (("threshold_db", math.nan), ("threshold_db", math.inf), ("threshold_db", -500.0), ("ratio", 0.5), ("ratio", math.nan),
                      ("ratio", -math.inf), ("knee_db", -1.0), ("knee_db", math.inf), ("attack_ms", 0.0), ("attack_ms", -5.0),
                      ("attack_ms", math.nan), ("release_ms", 0.0), ("release_ms", math.inf), ("makeup_db", math.nan), ("makeup_db", 1e9),
                      ("sample_rate", 0), ("sample_rate", math.nan)):
        with pytest.raises(ValueError, match=name):
            P.DynamicRangeOperator(**{name: bad})
    assert constants.MUSIC_DECOMPRESSION == "music_decompression"
    with pytest.raises((RuntimeError, AssertionError)):
        op.forward(torch.zeros(2, 640))                            # no CPU fallback


def test_pipeline_accepts_lanes_and_shards():
    """the operator keeps no per-clip state: the pipeline's own check of positional state passes for lanes and for shards, alone and as the
    inner operator (a track or a mixture around it is refused by THEIR checks, as for every inner operator)"""
    from types import SimpleNamespace
    from diffmusic_amd.pipelines.pipeline_musicldm import MusicLDMPipeline
    from diffmusic_amd import inverse_problem as P

    def check(op, **kw):
        pipe = SimpleNamespace(scheduler=SimpleNamespace(operator=op), lanes=kw.get("own_lanes", 1))
        return MusicLDMPipeline._check_positional_state(pipe, kw.get("shard", False), kw.get("group"), kw.get("lanes"))
    op = P.DynamicRangeOperator()
    track = P.TrackOperator(op, P.TrackLayout(11200, 6400, 1600))
    for o in (op, track, P.MixtureOperator(op, 2)):
        assert check(o) is None and check(o, lanes=2) is None and check(o, shard=True) is None and check(o, group=object()) is None
        assert check(o, own_lanes=3) is None


def test_abi_surface_lists_the_new_entry_points():
    from diffmusic_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "diffmusic_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    torch_ops = open(os.path.join(ROOT, "diffmusic_amd", "csrc_torch", "torch_ops.cpp")).read()
    for name in ("dmx_drc_fwd", "dmx_drc_bwd"):
        assert name in _lib._SIGS and name in _lib.ADDED_IN_V4
        assert re.search(rf"\b{name}\s*\(", header), name
        assert f"#pragma weak {name}\n" in torch_ops, name
    assert _lib.ABI_VERSION == 4 and "#define DMX_ABI_VERSION 4 " in header
    assert "drc_fwd" in ops.OP_NAMES and "drc_bwd" in ops.OP_NAMES
    with pytest.raises((RuntimeError, AssertionError)):
        ops.ctypes_hip.drc_fwd(torch.zeros(1, 300), 300, *D.PARAMS["base"].args)          # no CPU fallback


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
    assert mod.DECOMPRESSION == constants.MUSIC_DECOMPRESSION and mod.DECOMPRESSION in mod.TASKS
    t = ("-t", "music_decompression")

    def kw(*argv, cfg=None):
        return mod.compressor_params(mod.parse_args(list(argv)), cfg)
    assert kw(*t) == {}
    assert kw(*t, "--drc_ratio", "inf", "--drc_threshold_db", "-30") == {"ratio": math.inf, "threshold_db": -30.0}
    full = kw(*t, "--drc_threshold_db", "-18", "--drc_ratio", "8", "--drc_knee_db", "0", "--drc_attack_ms", "1", "--drc_release_ms", "50",
              "--drc_makeup_db", "6")
    assert full == dict(threshold_db=-18.0, ratio=8.0, knee_db=0.0, attack_ms=1.0, release_ms=50.0, makeup_db=6.0)
    for bad in (("--drc_ratio", "0.5"), ("--drc_ratio", "nan"), ("--drc_knee_db", "-1"), ("--drc_attack_ms", "0"), ("--drc_release_ms", "-3"),
                ("--drc_makeup_db", "inf"), ("--drc_threshold_db", "nan"), ("--drc_ratio", "four")):
        with pytest.raises(SystemExit):
            kw(*t, *bad)
    for other in ("music_inpainting", "music_declipping"):
        assert kw("-t", other) is None
        for flag in mod.DRC_FLAGS:
            with pytest.raises(SystemExit, match="music_decompression"):
                kw("-t", other, f"--drc_{flag}", "2")
    args = mod.parse_args([*t, "--track_overlap_s", "1.28"])                    # track mode is allowed
    assert args.track_overlap_s == 1.28 and mod.spectral_boxes(args) is None and mod.separation_stems(args) is None
    cfg = compose("dps", overrides=["data=moises", "model=musicldm", f"inverse_problem={mod.DECOMPRESSION}"])
    assert cfg.inverse_problem.noise.name == "gaussian" and float(cfg.inverse_problem.noise.sigma) == 0.0
    from_cfg = kw(*t, cfg=cfg)
    assert from_cfg == dict(threshold_db=-24.0, ratio=4.0, knee_db=6.0, attack_ms=5.0, release_ms=100.0, makeup_db=0.0)
    assert kw(*t, "--drc_ratio", "inf", cfg=cfg)["ratio"] == math.inf          # flags win
    op, scale = mod.build_operator(mod.DECOMPRESSION, cfg, "box", drc=kw(*t, "--drc_makeup_db", "3", cfg=cfg))
    assert isinstance(op, P.DynamicRangeOperator) and scale == 1 and op.makeup_db == 3.0 and op.sample_rate == cfg.data.sample_rate
    assert op.noiser is not None
    with pytest.raises(ValueError):
        mod.build_operator(mod.DECOMPRESSION, cfg, "box")
