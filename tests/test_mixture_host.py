"""CPU: the host side of source separation (diffmusic_amd/inverse_problem/mixture.py and the pipeline's mixture branch) -- the construction
rules of `MixtureOperator`, what it hands to the inner operator, the scheduler's refusal of per-clip norms, the pipeline's refusals and
output shapes on the CPU stand-ins of tests/stubs.py, the SI-SDR closed forms, the example's argument rules and the YAML."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests.stubs import SCHED, make_pipeline
from tests.test_track_host import _Inner, weights64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dmx_stem_mix_fwd", "dmx_stem_mix_bwd", "dmx_stem_project")
NEW_OPS = ("stem_mix_fwd", "stem_mix_bwd", "stem_project")


# ---- MixtureOperator ------------------------------------------------------------------------------------------------------------------
def test_construction_rules():
    from diffmusic_amd import inverse_problem as P
    op = P.MixtureOperator(_Inner(), 3, gains=(2.0, 0.25, 1.0))
    assert op.num_stems == 3 and op.gains == [2.0, 0.25, 1.0] and op.groups == 1 and op.num_clips == 3 and op.track is None
    assert P.MixtureOperator(_Inner(), 1).gains is None and P.MixtureOperator(_Inner(), 16).num_stems == 16
    assert P.MixtureOperator(_Inner(), 2, gains=torch.tensor([1.0, -0.5])).gains == [1.0, -0.5]
    with pytest.raises(ValueError, match="around a MixtureOperator"):
        P.MixtureOperator(op, 3)
    style = object.__new__(P.StyleGuidanceOperator)                                   # no tower is built: the type alone is refused
    with pytest.raises(ValueError, match="StyleGuidanceOperator"):
        P.MixtureOperator(style, 3)
    for bad in (0, 17, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="num_stems"):
            P.MixtureOperator(_Inner(), bad)
    with pytest.raises(ValueError, match="2 gains for 3 stems"):
        P.MixtureOperator(_Inner(), 3, gains=(1.0, 1.0))
    for bad in (float("nan"), float("inf"), 1e39):                                    # 1e39 is finite in float64, not in fp32
        with pytest.raises(ValueError, match="finite"):
            P.MixtureOperator(_Inner(), 3, gains=(1.0, bad, 1.0))
    with pytest.raises(ValueError, match="global noise stream"):
        P.MixtureOperator(_Inner(noiser=P.GaussianNoise(0.05, stream="clip")), 3)
    P.MixtureOperator(_Inner(noiser=P.GaussianNoise(0.0, stream="clip")), 3)          # sigma 0 draws nothing: no stream to refuse
    P.MixtureOperator(_Inner(noiser=P.GaussianNoise(0.05)), 3)


def test_delegation_and_the_one_sample_property():
    from diffmusic_amd import inverse_problem as P
    inner = _Inner(noiser=P.GaussianNoise(0.05))
    inner.dead_span = lambda length: (10, length - 10)
    op = P.MixtureOperator(inner, 3)
    x = torch.arange(6.0)[None]
    assert torch.equal(op.transform(x), x + 1.0) and torch.equal(op.inverse_transform(x, lambda m: m - 1.0), x - 1.0)
    assert op.noiser is inner.noiser and op.cache_reference is True and op.dead_span(100) == (10, 90)
    op.reset_cache()
    op.restart()                                                                      # the inner stand-in has none: a no-op
    assert inner.resets == 1
    assert P.MixtureOperator(_Inner(), 2).dead_span(100) is None                      # an inner operator without the method
    lay = P.TrackLayout(16000, 6400, 1600)
    nested = P.MixtureOperator(P.TrackOperator(_Inner(), lay), 4)
    assert nested.groups == 3 and nested.num_clips == 12 and nested.track is nested.inner and nested.dead_span(6400) is None
    # one property says "the batch is one sample" on both wrappers, and nothing else carries it
    assert "one sample" in op.one_sample and "one sample" in nested.inner.one_sample and op.one_sample != nested.inner.one_sample
    assert getattr(_Inner(), "one_sample", None) is None and getattr(P.IdentityOperator, "one_sample", None) is None
    with pytest.raises(RuntimeError, match="GPU only"):
        op.forward(torch.zeros(3, 64))                                                # no CPU fallback
    with pytest.raises(ValueError, match="expected \\(3, >= 6400\\)"):
        op.guidance(torch.zeros(2, 6432), 6400, None, "mel_spectrogram")
    inner.noiser = P.GaussianNoise(0.05, stream="clip")                               # swapped in later: refused when used
    with pytest.raises(ValueError, match="global noise stream"):
        op.guidance(torch.zeros(3, 6432), 6400, None, "mel_spectrogram")


def test_project_is_refused_off_the_plain_clean_mixture():
    from diffmusic_amd import inverse_problem as P
    with pytest.raises(ValueError, match="not the mixture itself"):
        P.MixtureOperator(_Inner(), 3).project(torch.zeros(3, 64), torch.zeros(1, 64))
    ident = object.__new__(P.IdentityOperator)                                        # no front end is built: host checks only
    ident.noiser = P.GaussianNoise(0.05)
    with pytest.raises(ValueError, match="sigma > 0"):
        P.MixtureOperator(ident, 3).project(torch.zeros(3, 64), torch.zeros(1, 64))
    ident.noiser = None
    with pytest.raises(RuntimeError, match="GPU only"):
        P.MixtureOperator(ident, 3).project(torch.zeros(3, 64), torch.zeros(1, 64))


def test_new_entry_points_are_additive_and_bound_in_both_bindings():
    from diffmusic_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "diffmusic_hip.h")).read()
    src = open(os.path.join(ROOT, "diffmusic_amd", "csrc_torch", "torch_ops.cpp")).read()
    assert "#define DMX_ABI_VERSION 4 " in hdr and _lib.ABI_VERSION == 4
    for s in NEW_SYMBOLS:
        assert s in _lib._SIGS and s in _lib.ADDED_IN_V4 and f"int {s}(" in hdr and f"#pragma weak {s}" in src, s
    for name in NEW_OPS:
        assert name in ops.OP_NAMES and f'm.def("{name}(' in src, name
    h = ops.load()                                                                    # no CPU fallback, in either binding
    for b in (h, ops.ctypes_hip):
        with pytest.raises(RuntimeError, match="GPU tensor"):
            b.stem_mix_fwd(torch.zeros(2, 8), None, 2, 1, 8)
        with pytest.raises(RuntimeError, match="GPU tensor"):
            b.stem_mix_bwd(torch.zeros(1, 8), None, 2, 8)
        with pytest.raises(RuntimeError, match="GPU tensor"):
            b.stem_project(torch.zeros(2, 8), torch.zeros(1, 8), None, 8)


def test_scheduler_refuses_per_clip_norms_for_a_mixture():
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    x = torch.zeros(3, 8, 10, 16)
    for op in (P.MixtureOperator(_Inner(), 3), P.MixtureOperator(P.TrackOperator(_Inner(), P.TrackLayout(6400, 6400, 1600)), 3)):
        s = get_scheduler("dps")(operator=op, **SCHED)
        s.set_timesteps(10)
        with pytest.raises(ValueError, match="MixtureOperator makes the batch one sample.*per_clip_norm=False"):
            s.step(x, s._timesteps_host[0], x)


# ---- the pipeline's mixture branch on the CPU stand-ins ---------------------------------------------------------------------------------
N, SECONDS, L = 6, 0.64, 10240            # as tests/test_track_host.py: latent (B, 8, 16, 4), windows of 10240 samples


def _cpu_track(lay, inner=None):
    from diffmusic_amd import inverse_problem as P

    class CpuTrackOperator(P.TrackOperator):
        """The stitch launch replaced by its torch restatement (tests/test_track_host.py)."""

        def stitch(self, wav):
            wt = torch.from_numpy(weights64(self.layout))
            out = torch.zeros(self.layout.track_len, dtype=torch.float64)
            for w, s in enumerate(self.layout.starts):
                out[s:s + L] += wt[w, s:s + L] * wav[w, :L].double()
            return out.float()[None]
    return CpuTrackOperator(inner if inner is not None else _Inner(), lay)


def _mix_pipe(K=3, T=None, inner=None, per_clip_norm=False):
    from diffmusic_amd import inverse_problem as P
    pipe = make_pipeline(per_clip_norm=per_clip_norm)
    lay = P.TrackLayout(T, L, 2560) if T is not None else None
    inner = inner if inner is not None else _Inner()
    pipe.scheduler.operator = P.MixtureOperator(inner if lay is None else _cpu_track(lay, inner), K, gains=[2.0, 0.25, 1.0][:K])
    return pipe, lay


def _call(pipe, B, **kw):
    pe = torch.randn(B, 512, generator=torch.Generator().manual_seed(99))
    args = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N, show_progress=False, eta=0.0,
                generator=[torch.Generator().manual_seed(s) for s in range(B)])
    args.update(kw)
    return pipe(**args)


def test_pipeline_returns_the_stems():
    pipe, _ = _mix_pipe()
    out = _call(pipe, 3)
    assert out.audios.shape == (3, L) and out.audios.dtype == np.float32 and np.isfinite(out.audios).all()
    assert len(pipe.last_losses) == N and pipe.scheduler.operator.inner.resets >= 1
    plain = make_pipeline(per_clip_norm=False)
    assert np.array_equal(out.audios, _call(plain, 3).audios)                          # the existing output stage, unchanged
    assert _call(pipe, 3, output_type="latent").audios.shape == (3, 8, 16, 4)


def test_pipeline_stitches_every_stem_of_a_track():
    pipe, lay = _mix_pipe(K=2, T=25600)
    assert lay.num_windows == 3
    out = _call(pipe, 6)
    assert out.audios.shape == (2, lay.track_len)
    assert _call(pipe, 6, output_type="latent").audios.shape == (6, 8, 16, 4)          # the K * W latents
    wins = torch.from_numpy(_call(make_pipeline(per_clip_norm=False), 6).audios)
    track = pipe.scheduler.operator.track
    want = torch.cat([track.stitch(wins[0:3]), track.stitch(wins[3:6])]).numpy()       # stem-major: stem k owns rows k W .. k W + W - 1
    assert np.array_equal(out.audios, want)


def test_pipeline_mixture_refusals():
    from diffmusic_amd import inverse_problem as P
    pipe, _ = _mix_pipe()
    with pytest.raises(ValueError, match="holds 2 clips, but the mixture has 3 stems"):
        _call(pipe, 2)
    with pytest.raises(ValueError, match="sharded"):
        _call(pipe, 3, shard=True)
    with pytest.raises(ValueError, match="sharded"):
        _call(pipe, 3, group=object())
    with pytest.raises(ValueError, match="lanes"):
        _call(pipe, 3, lanes=2)
    pipe.lanes = 3
    with pytest.raises(ValueError, match="lanes"):
        _call(pipe, 3)
    pipe.lanes = 1
    clipnorm, _ = _mix_pipe(per_clip_norm=True)
    with pytest.raises(ValueError, match="per_clip_norm=False"):
        _call(clipnorm, 3)
    noisy, _ = _mix_pipe()
    noisy.scheduler.operator.inner.noiser = P.GaussianNoise(0.05, stream="clip")
    with pytest.raises(ValueError, match="global noise stream"):
        _call(noisy, 3)
    noisy.scheduler.operator.inner.noiser = P.GaussianNoise(0.05, stream="global")    # the global stream is allowed
    assert _call(noisy, 3).audios.shape == (3, L)
    nested, lay = _mix_pipe(K=2, T=25600)
    with pytest.raises(ValueError, match="holds 3 clips, but the mixture has 2 stems of 3 windows"):
        _call(nested, 3)                                                              # K * W rows, not W
    with pytest.raises(ValueError, match="window_len"):
        _call(nested, 6, audio_length_in_s=0.32)
    for p in (pipe, clipnorm, nested):
        assert p.scheduler.calls == 0                                                 # every refusal came before the first step


def test_positional_state_is_found_through_both_wrappers():
    """`Mixture(Track(BlindDereverberation))`: the response estimates are indexed by batch position, so lanes and shards are refused with
    the blind operator's own message only if the check unwraps every wrapper (the mixture's rules are switched off to reach it)."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.pipelines.pipeline_musicldm import MusicLDMPipeline
    pipe, _ = _mix_pipe(K=2, T=25600, inner=P.BlindDereverberationOperator(ir_length=64))
    pipe._check_mixture = lambda *a, **k: None
    with pytest.raises(ValueError, match="BlindDereverberationOperator cannot run as clip lanes"):
        _call(pipe, 6, lanes=2)
    with pytest.raises(ValueError, match="BlindDereverberationOperator cannot be sharded"):
        _call(pipe, 6, shard=True)
    assert MusicLDMPipeline._check_mixture is not pipe._check_mixture


def test_a_call_without_a_mixture_never_reaches_the_mixture_branch(monkeypatch):
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.pipelines.pipeline_musicldm import MusicLDMPipeline
    reached = []
    monkeypatch.setattr(MusicLDMPipeline, "_check_mixture", lambda self, *a, **k: reached.append("check"))
    monkeypatch.setattr(P.MixtureOperator, "stitch_stems", lambda self, wav: reached.append("stitch"))
    for op in (None, _Inner()):
        pipe = make_pipeline(per_clip_norm=False)
        pipe.scheduler.operator = op
        assert _call(pipe, 3).audios.shape == (3, L)
    pipe = make_pipeline(per_clip_norm=False)
    lay = P.TrackLayout(25600, L, 2560)
    pipe.scheduler.operator = _cpu_track(lay)
    assert _call(pipe, 3).audios.shape == (1, lay.track_len)                          # track mode is the track's own branch
    assert reached == []


# ---- SI-SDR ---------------------------------------------------------------------------------------------------------------------------
def _orthogonal_pair(n=4000, seed=3):
    g = np.random.default_rng(seed)
    s, r = g.standard_normal(n), g.standard_normal(n)
    return s, r - (r @ s) / (s @ s) * s                                               # n is orthogonal to s in float64


def test_sisdr_closed_forms():
    from diffmusic_amd.metrics import ScaleInvariantSDR
    m = ScaleInvariantSDR()
    s, n = _orthogonal_pair()
    assert m.max_db == 100.0
    for a in (1.0, 0.3, -2.0):                                                        # s_hat = a s: nothing but the target, the documented clamp
        assert m.score([s], [a * s])[0] == 100.0
    assert ScaleInvariantSDR(max_db=60.0).score([s], [0.5 * s])[0] == 60.0
    for scale in (1.0, 0.1, 3.0):
        want = 10 * math.log10((s @ s) / ((scale * n) @ (scale * n)))
        got = m.score([s], [s + scale * n])[0]
        assert abs(got - want) < 1e-5, (got, want)
        for c in (0.01, 7.0, -1.0):                                                   # invariant to the scale of the estimate
            assert abs(m.score([s], [c * (s + scale * n)])[0] - want) < 1e-5
    assert m.score([s], [n])[0] == -100.0                                             # orthogonal estimate: no target at all
    assert math.isnan(m.score([np.zeros(8)], [np.ones(8)])[0])                        # silent reference
    both = m.score([s, s[:2000]], [s + n, (s + 0.5 * n)[:3000]])                      # per clip, on the common prefix
    assert both.shape == (2,) and both.dtype == np.float64
    assert abs(ScaleInvariantSDR("mean").score([s, s], [s + n, s + 0.1 * n]) - np.mean(m.score([s, s], [s + n, s + 0.1 * n]))) < 1e-12
    with pytest.raises(AssertionError):
        ScaleInvariantSDR("sum")


# ---- the example and the config -------------------------------------------------------------------------------------------------------
def _example():
    spec = importlib.util.spec_from_file_location("run_inverse_problem", os.path.join(ROOT, "examples", "run_inverse_problem.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_yaml_loads():
    from diffmusic_amd import constants
    from diffmusic_amd.config import compose
    assert constants.MUSIC_SOURCE_SEPARATION == "music_source_separation"
    cfg = compose("dps", overrides=["data=moises", "model=musicldm", "inverse_problem=music_source_separation"])
    assert cfg.inverse_problem.name == "music_source_separation"
    assert cfg.inverse_problem.noise.name == "gaussian" and cfg.inverse_problem.noise.sigma == 0.0


def test_example_argument_rules():
    mod = _example()
    t = ["-t", "music_source_separation"]
    assert "music_source_separation" in mod.TASKS

    def stems(*argv):
        return mod.separation_stems(mod.parse_args(list(argv)))
    assert stems(*t) == 2                                                             # two synthetic stems
    assert stems(*t, "--wav", "a.wav", "b.wav", "c.wav") == 3
    assert stems(*t, "--wav", "a.wav", "b.wav", "--gains", "1", "0.5", "--project", "--track_overlap_s", "1.28") == 2
    assert stems(*t, "--mixture", "mix.wav", "--stems", "4") == 4
    args = mod.parse_args(t + ["--stems", "3", "--gains", "2", "0.25", "1"])
    assert args.gains == [2.0, 0.25, 1.0] and mod.separation_stems(args) == 3
    for argv, msg in (((*t, "--mixture", "mix.wav"), "needs --stems"),
                      ((*t, "--mixture", "mix.wav", "--stems", "2", "--wav", "a.wav"), "pass one of them"),
                      ((*t, "--wav", "a.wav", "b.wav", "--stems", "3"), "every --wav is one stem"),
                      ((*t, "--stems", "17"), "1 .. 16"),
                      ((*t, "--stems", "0"), "1 .. 16"),
                      ((*t, "--stems", "3", "--gains", "1", "1"), "2 values for 3 stems"),
                      ((*t, "--batch", "2"), "one mixture per call"),
                      (("-t", "music_inpainting", "--gains", "1"), "belongs to -t music_source_separation"),
                      (("-t", "music_inpainting", "--mixture", "m.wav"), "belongs to"),
                      (("-t", "music_declipping", "--stems", "2"), "belongs to")):
        with pytest.raises(SystemExit, match=msg):
            stems(*argv)
    assert stems("-t", "music_inpainting") is None                                    # every other task: untouched
