"""CPU: the float64 model, the element-wise bound, the fp32 emulation and the mutants of the time-frequency gain (tests/tf_gain_cases.py),
the host helpers of inverse_problem/dsp.py, the operator's constructor and dead span, and the example's argument rules.  The GPU side
(tests/test_gpu_tf_gain.py) compares the kernel with the same model under the same bound."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import tf_gain_cases as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("c", TF.CASES, ids=lambda c: c.name)
def test_emulation_lies_within_the_bound_in_every_element(c):
    r = TF.run_case(c)
    print(f"{c.name}: largest |emulation - model| / bound = {r:.4f}")
    assert r <= 1.0, (c.name, r)


@pytest.mark.parametrize("name", sorted(TF.MUTANTS))
def test_every_mutant_leaves_the_bound(name):
    where, cases = TF.MUTANTS[name]
    ratios = {cn: TF.run_case(TF.CASE[cn], name, where) for cn in cases}
    print(name, ratios)
    assert max(ratios.values()) > 1.0, (name, ratios)


def test_case_table_covers_the_branches():
    Ls = {c.L for c in TF.CASES}
    assert {300, 1024, 1025, TF.SLAB, TF.SLAB + 1, 4999, 6400} <= Ls
    assert TF.frames(300) == 5
    kinds = {(c.gain, c.per_clip) for c in TF.CASES}
    for g in ("ones", "rand", "bin0", "bin1", "bin511", "bin512", "frame_first", "frame_last", "frame_edge", "zero_frames"):
        assert any(k[0] == g for k in kinds), g
    assert any(c.stride == 6432 and c.L == 6400 and c.full > c.L for c in TF.CASES)
    i = TF.inputs(TF.CASE["L4999_edge"])
    assert np.signbit(i.x[0, 17]) and i.x[0, 17] == 0 and np.abs(i.x).max() >= 1e4


@pytest.mark.parametrize("L", [300, 1025, 4999])
def test_model_is_the_identity_for_unit_gain(L):
    x = np.random.default_rng(L).standard_normal((2, L))
    y = TF.model(x, np.ones((TF.NB, TF.frames(L))), L).y
    assert np.abs(y - x).max() <= 1e-12


@pytest.mark.parametrize("L,per_clip", [(300, False), (2049, True), (4999, False)])
def test_model_is_symmetric(L, per_clip):
    rng = np.random.default_rng(L + 1)
    x, y = rng.standard_normal((2, L)), rng.standard_normal((2, L))
    G = rng.uniform(-1.0, 2.0, ((2,) if per_clip else ()) + (TF.NB, TF.frames(L)))
    Ax, Ay = TF.model(x, G, L).y, TF.model(y, G, L).y
    for b in range(2):
        lhs, rhs = float(Ax[b] @ y[b]), float(x[b] @ Ay[b])
        scale = float(np.abs(Ax[b]) @ np.abs(y[b]) + np.abs(x[b]) @ np.abs(Ay[b]))
        assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)


def test_window_constant_is_exactly_one_and_a_half():
    w = TF.window()
    c = (w.reshape(4, 256) ** 2).sum(0)
    assert np.abs(c - 1.5).max() < 1e-14


# ---- host helpers (inverse_problem/dsp.py)
def test_tf_frames():
    from diffmusic_amd.inverse_problem import tf_frames
    assert [tf_frames(L) for L in (1, 256, 257, 300, 1024, 1025, 6400, 160000)] == [4, 4, 5, 5, 7, 8, 28, 628]
    with pytest.raises(ValueError):
        tf_frames(0)


def test_tf_gain_grid_against_hand_computed_grids():
    from diffmusic_amd.inverse_problem import tf_gain_grid
    sr, L = 16000, 6400                                      # bins 15.625 Hz apart; frame centres at (t - 1) * 0.016 s
    g = tf_gain_grid(L, sr, [(1000.0, 2000.0, None, None, 0.0)])
    assert g.shape == (513, 28) and g.dtype == np.float32
    assert (g[64:129] == 0).all() and (g[:64] == 1).all() and (g[129:] == 1).all()      # 64 * 15.625 = 1000, 128 * 15.625 = 2000 inclusive
    g = tf_gain_grid(L, sr, [(None, None, 0.1, 0.2, 0.25)], base=2.0)
    cols = [t for t in range(28) if 0.1 <= (t - 1) * 0.016 < 0.2]               # centres ((t - 3) 256 + 512) / 16000 = (t - 1) * 0.016
    assert cols == list(range(8, 14))
    assert (g[:, cols] == 0.25).all() and (np.delete(g, cols, axis=1) == 2.0).all()
    g = tf_gain_grid(L, sr, [(None, 500.0, None, 0.05, 0.0), (0.0, 100.0, 0.0, None, 3.0)])    # later boxes overwrite earlier ones
    assert (g[:7, 1:] == 3.0).all() and (g[7:33, :5] == 0).all() and (g[:7, 0] == 0).all() and (g[33:] == 1).all() and (g[7:33, 5:] == 1).all()
    with pytest.raises(ValueError):
        tf_gain_grid(L, sr, [(0.0, 1.0, None, None, math.inf)])
    with pytest.raises(ValueError):
        tf_gain_grid(L, sr, [(0.0, 1.0, None, None)])


def test_hum_boxes():
    from diffmusic_amd.inverse_problem import hum_boxes, tf_gain_grid
    assert hum_boxes(50.0, 3, 20.0) == [(40.0, 60.0, None, None, 0.0), (90.0, 110.0, None, None, 0.0), (140.0, 160.0, None, None, 0.0)]
    g = tf_gain_grid(6400, 16000, hum_boxes(50.0, 2, 32.0))
    zero_bins = sorted(set(np.flatnonzero((g == 0).all(1)).tolist()))
    assert zero_bins == [3, 4, 6, 7]                          # 46.9, 62.5 | 93.75, 109.4 Hz
    with pytest.raises(ValueError):
        hum_boxes(0.0, 1, 4.0)
    with pytest.raises(ValueError):
        hum_boxes(50.0, 0, 4.0)


# ---- the operator without a GPU
def _op(gain, **kw):
    from diffmusic_amd.inverse_problem import TimeFrequencyMaskOperator
    return TimeFrequencyMaskOperator(16000, gain, **kw)


def test_constructor_refusals_need_no_gpu():
    T = 28
    op = _op(np.ones((513, T), np.float32))
    assert not op.per_clip and op.frames == T and op.dead_span(6400) is None
    assert _op(torch.ones(3, 513, T)).per_clip
    for bad in (np.ones(513), np.ones((512, T)), np.ones((2, 2, 513, T)), np.ones((T, 513))):
        with pytest.raises(ValueError, match="513"):
            _op(bad)
    for v in (math.nan, math.inf):
        g = np.ones((513, T), np.float32)
        g[5, 5] = v
        with pytest.raises(ValueError, match="finite"):
            _op(g)


def test_shape_errors_name_the_expected_shape_before_any_gpu_work():
    op = _op(np.ones((513, 28), np.float32))
    x = torch.zeros(2, 6401)                                  # T would be 29
    for call in (lambda: op.forward(x), lambda: op.apply(x, 6401), lambda: op.guidance(x, 6401, x, "wav_form")):
        with pytest.raises(ValueError, match=r"\(513, 29\)"):
            call()
    op = _op(np.ones((3, 513, 28), np.float32))
    x = torch.zeros(2, 6400)
    for call in (lambda: op.forward(x), lambda: op.apply(x, 6400), lambda: op.guidance(x, 6400, x, "mel_spectrogram")):
        with pytest.raises(ValueError, match=r"\(2, 513, 28\)"):
            call()


def test_dead_span_on_hand_made_grids():
    T, L = 28, 6400
    g = np.ones((513, T), np.float32)
    g[:, 8:11] = 0                                            # exactly 3 zero frames: no sample has all four of its frames zero
    assert _op(g).dead_span(L) is None
    g[:, 8:12] = 0                                            # 4 zero frames 8 .. 11: one hop, [256 * 8, 256 * 9)
    assert _op(g).dead_span(L) == (2048, 2304)
    g[:, 15:25] = 0                                           # the longest run wins: frames 15 .. 24 -> [3840, 5632)
    assert _op(g).dead_span(L) == (3840, 5632)
    assert _op(g).dead_span(L + 1) is None                   # another clip length: no claim
    g[100, 20] = 1e-30                                        # one non-zero bin splits the run: 15 .. 19 and 21 .. 24
    assert _op(g).dead_span(L) == (3840, 4352)
    pc = np.stack([g, g])
    pc[1, :, 15:25] = 1                                       # every clip has to be zero there
    assert _op(pc).dead_span(L) == (2048, 2304)
    g = np.ones((513, T), np.float32)
    g[:, 22:] = 0                                             # up to the last frame: the span ends with the clip
    assert _op(g).dead_span(L) == (5632, 6400)
    g = np.ones((513, T), np.float32)
    g[:, :5] = 0                                              # from the first frame
    assert _op(g).dead_span(L) == (0, 512)
    g = -np.zeros((513, T), np.float32)                       # -0.0 is zero
    assert _op(g).dead_span(L) == (0, 6400)


def test_dead_samples_are_exactly_zero_in_the_model_and_their_bound_is_zero():
    c = TF.CASE["L6400_zero_frames"]
    r, q = TF.reference(c)
    assert (r.y[:, 1536:2560] == 0).all() and (q[:, 1536:2560] == 0).all()      # frames 6 .. 12 -> [256 * 6, 256 * 10)
    op = _op(TF.inputs(c).gain)
    assert op.dead_span(6400) == (1536, 2560)
    x = TF.inputs(c).x.astype(np.float64).copy()
    x[:, 1536:2560] += 1.0                                    # A does not see those samples (the dead span's other half)
    assert np.abs(TF.model(x, TF.inputs(c).gain, 6400).y - r.y).max() <= 1e-13


def test_pipeline_refuses_lanes_and_shards_for_per_clip_gains_only():
    from diffmusic_amd.pipelines.pipeline_musicldm import MusicLDMPipeline
    from types import SimpleNamespace
    T = 28

    def check(op, **kw):
        pipe = SimpleNamespace(scheduler=SimpleNamespace(operator=op), lanes=1)
        return MusicLDMPipeline._check_positional_state(pipe, kw.get("shard", False), kw.get("group"), kw.get("lanes"))
    shared, per_clip = _op(np.ones((513, T), np.float32)), _op(np.ones((2, 513, T), np.float32))
    check(shared, lanes=2)
    check(shared, shard=True)
    check(per_clip)
    with pytest.raises(ValueError, match="lanes"):
        check(per_clip, lanes=2)
    with pytest.raises(ValueError, match="shard"):
        check(per_clip, shard=True)


# ---- examples/run_inverse_problem.py
def _example():
    spec = importlib.util.spec_from_file_location("run_inverse_problem", os.path.join(ROOT, "examples", "run_inverse_problem.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_argument_rules():
    mod = _example()
    assert "music_spectral_inpainting" in mod.TASKS

    def boxes(*argv, cfg=None):
        return mod.spectral_boxes(mod.parse_args(list(argv)), cfg)
    t = ("-t", "music_spectral_inpainting")
    assert boxes(*t, "--tf_box", "2000,4000,2,2.5") == [(2000.0, 4000.0, 2.0, 2.5, 0.0)]
    assert boxes(*t, "--tf_box", ",4000,,2.5,0.5", "--tf_box", "none,None,1,,-1") == [(None, 4000.0, None, 2.5, 0.5), (None, None, 1.0, None, -1.0)]
    assert boxes(*t, "--hum", "50") == [(34.0, 66.0, None, None, 0.0)]
    assert boxes(*t, "--hum", "60,2,10", "--tf_box", "0,100,0,1,1") == [(55.0, 65.0, None, None, 0.0), (115.0, 125.0, None, None, 0.0),
                                                                         (0.0, 100.0, 0.0, 1.0, 1.0)]
    for bad in (("--tf_box", "1,2,3"), ("--tf_box", "1,2,3,4,5,6"), ("--tf_box", "a,2,3,4"), ("--tf_box", "3000,2000,0,1"), ("--tf_box", "0,1,2,2"),
                ("--tf_box", "0,1,0,1,"), ("--tf_box", "0,1,0,1,inf"), ("--hum", "0"), ("--hum", "50,1.5"), ("--hum", "50,0"), ("--hum", "50,1,-1"),
                ("--hum", "50,1,2,3"), ()):
        with pytest.raises(SystemExit):
            boxes(*t, *bad)
    for other in ("music_inpainting", "music_declipping"):
        assert boxes("-t", other) is None
        with pytest.raises(SystemExit, match="music_spectral_inpainting"):
            boxes("-t", other, "--tf_box", "0,1,0,1")
        with pytest.raises(SystemExit, match="music_spectral_inpainting"):
            boxes("-t", other, "--hum", "50")


def test_example_takes_its_boxes_from_the_config_and_builds_the_operator():
    from diffmusic_amd.config import compose
    from diffmusic_amd import constants, inverse_problem as P
    mod = _example()
    assert constants.MUSIC_SPECTRAL_INPAINTING == mod.SPECTRAL
    cfg = compose("dps", overrides=["data=moises", "model=musicldm", f"inverse_problem={mod.SPECTRAL}"])
    assert cfg.inverse_problem.noise.name == "gaussian" and float(cfg.inverse_problem.noise.sigma) == 0.0
    args = mod.parse_args(["-t", mod.SPECTRAL])
    bx = mod.spectral_boxes(args, cfg)
    assert bx == [(2000.0, 4000.0, 2.0, 2.5, 0.0)]
    op, scale = mod.build_operator(mod.SPECTRAL, cfg, "box", tf_boxes=bx)
    sr = cfg.data.sample_rate
    L = int(cfg.model.pipe.audio_length_in_s * sr)
    assert isinstance(op, P.TimeFrequencyMaskOperator) and scale == 1 and tuple(op.gain.shape) == (513, P.tf_frames(L))
    assert torch.equal(op.gain, torch.from_numpy(P.tf_gain_grid(L, sr, bx)))
    assert mod.spectral_boxes(mod.parse_args(["-t", mod.SPECTRAL, "--hum", "50"]), cfg) == [(34.0, 66.0, None, None, 0.0)]   # flags win
    with pytest.raises(ValueError):
        mod.build_operator(mod.SPECTRAL, cfg, "box")


def test_abi_surface_lists_the_new_entry_points():
    from diffmusic_amd import _lib, ops
    assert "dmx_audio_tf_gain" in _lib._SIGS and "dmx_audio_tf_frames" in _lib._SIGS
    assert "dmx_audio_tf_gain" in _lib.ADDED_IN_V4 and _lib.ABI_VERSION == 4
    assert "tf_gain" in ops.OP_NAMES
    with pytest.raises((RuntimeError, AssertionError)):
        ops.ctypes_hip.tf_gain(0, torch.zeros(1, 300), torch.ones(5, 513), 300, 300)       # no CPU fallback
