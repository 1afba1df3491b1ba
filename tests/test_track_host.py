"""CPU: track mode's host side (diffmusic_amd/inverse_problem/track.py and the pipeline's track branch) -- the layout rules over a
sweep of (T, L, R) against a float64 restatement of the formulas, the refusals of `TrackLayout` / `TrackOperator`, the scheduler's
refusal of per-clip norms, and, on the CPU stand-ins of tests/stubs.py, the pipeline's refusals and the shape of the returned track."""
import math

import numpy as np
import pytest
import torch

from tests.stubs import make_pipeline

NEW_SYMBOLS = ("dmx_track_stitch_fwd", "dmx_track_stitch_bwd")
NEW_OPS = ("track_stitch_fwd", "track_stitch_bwd")


def weights64(layout):
    """The (W, T) float64 matrix of S: weights64[w, n] = u(n - start[w]) / den[n] on the samples window w covers, 0 elsewhere."""
    T, L, R = layout.track_len, layout.window_len, layout.overlap
    i = np.arange(L, dtype=np.float64)
    u = np.minimum(np.minimum(i + 0.5, L - 0.5 - i), float(R)) / float(R)
    m = np.zeros((layout.num_windows, T), dtype=np.float64)
    for w, s in enumerate(layout.starts):
        m[w, s:s + L] = u
    return m / m.sum(axis=0, keepdims=True)


SWEEP = [(6400, 6400, 1600), (6401, 6400, 1600), (11300, 6400, 1600), (16000, 6400, 1600), (16000, 6400, 3200), (12800, 6400, 3200),
         (9600, 6400, 3200), (100000, 6400, 1), (1167360, 163840, 20480), (20, 8, 4), (21, 8, 3), (9, 8, 1), (1000, 10, 5), (37, 7, 3)]


@pytest.mark.parametrize("T,L,R", SWEEP)
def test_layout_rules(T, L, R):
    from diffmusic_amd.inverse_problem import TrackLayout
    lay = TrackLayout(T, L, R)
    W = lay.num_windows
    assert W == (1 if T == L else 1 + math.ceil((T - L) / (L - R))) and len(lay.starts) == W
    assert lay.starts[0] == 0 and lay.starts[-1] == T - L
    assert lay.starts == ([0] if W == 1 else [(w * (T - L)) // (W - 1) for w in range(W)])
    cover = np.zeros(T, dtype=np.int64)
    for s in lay.starts:
        assert 0 <= s <= T - L
        cover[s:s + L] += 1
    assert cover.min() >= 1                                                          # every sample is covered
    for a, b in zip(lay.starts, lay.starts[1:]):
        assert b > a and a + L - b >= R, (a, b)                                      # consecutive windows overlap by at least R
    wt = weights64(lay)
    assert np.abs(wt.sum(axis=0) - 1.0).max() <= 1e-12
    assert (wt[:, cover == 1].max(axis=0) == 1.0).all()                              # one covering window: weight exactly 1
    track = torch.arange(T, dtype=torch.float32)
    cut = lay.cut(track[None])
    assert cut.shape == (W, L) and all(torch.equal(cut[w], track[s:s + L]) for w, s in enumerate(lay.starts))
    assert torch.equal(lay.cut(track), cut)


def test_seconds_for_samples_round_trips():
    from diffmusic_amd.inverse_problem import seconds_for_samples
    for sr in (16000, 22050, 44100, 48000):
        for n in list(range(1, 3000)) + [163840, 288000, 299520, 1136640, 1167360, 1167361, 7654321]:
            assert int(seconds_for_samples(n, sr) * sr) == n, (n, sr)
    assert seconds_for_samples(160000, 16000) == 10.0


def test_three_windows_may_cover_a_sample():
    from diffmusic_amd.inverse_problem import TrackLayout
    lay = TrackLayout(11300, 6400, 1600)
    assert lay.starts == [0, 2450, 4900] and lay.num_windows == 3
    n = 5000
    assert sum(1 for s in lay.starts if s <= n < s + 6400) == 3
    lay = TrackLayout(1167360, 163840, 20480)
    assert lay.num_windows == 8 and lay.starts == [w * 143360 for w in range(8)]      # the headline size: overlap exactly R
    wt = weights64(TrackLayout(16000, 6400, 1600))                                    # starts 0, 4800, 9600: overlaps of exactly R
    n = np.arange(4800, 6400)
    assert np.allclose(wt[1, n], (n - 4800 + 0.5) / 1600, atol=1e-15) and np.allclose(wt[0, n], 1 - wt[1, n], atol=1e-15)


@pytest.mark.parametrize("T,L,R", [(6399, 6400, 1600), (0, 6400, 1600), (16000, 6400, 0), (16000, 6400, -5), (16000, 6400, 3201),
                                   (16000, 7, 4)])
def test_layout_refusals(T, L, R):
    from diffmusic_amd.inverse_problem import TrackLayout
    with pytest.raises(ValueError):
        TrackLayout(T, L, R)
    lay = TrackLayout(16000, 6400, 1600)
    with pytest.raises(ValueError, match="samples"):
        lay.cut(torch.zeros(1, 15999))


class _Inner:
    """A measurement operator as far as the host logic looks at it."""
    cache_reference = True

    def __init__(self, noiser=None):
        self.noiser, self.resets = noiser, 0

    def forward(self, data, **kw):
        return data * 2.0

    def transform(self, data):
        return data + 1.0

    def inverse_transform(self, mel, vocoder):
        return vocoder(mel)

    def reset_cache(self):
        self.resets += 1


def test_track_operator_delegates_and_refuses():
    from diffmusic_amd import inverse_problem as P
    lay = P.TrackLayout(16000, 6400, 1600)
    inner = _Inner(noiser=P.GaussianNoise(0.05))
    op = P.TrackOperator(inner, lay)
    x = torch.arange(6.0)[None]
    assert torch.equal(op.forward(x), x * 2.0) and torch.equal(op.transform(x), x + 1.0)
    assert torch.equal(op.inverse_transform(x, lambda m: m - 1.0), x - 1.0)
    assert op.noiser is inner.noiser and op.layout is lay and op.inner is inner
    op.reset_cache()
    assert inner.resets == 1
    with pytest.raises(ValueError, match="global noise stream"):
        P.TrackOperator(_Inner(noiser=P.GaussianNoise(0.05, stream="clip")), lay)
    P.TrackOperator(_Inner(noiser=P.GaussianNoise(0.0, stream="clip")), lay)          # sigma 0 draws nothing: no stream to refuse
    inner.noiser = P.GaussianNoise(0.05, stream="clip")                               # swapped in later: refused when used
    with pytest.raises(ValueError, match="global noise stream"):
        op.guidance(torch.zeros(3, 6432), 6400, None, "mel_spectrogram")
    with pytest.raises(ValueError, match="wrap the measurement operator"):
        P.TrackOperator(op, lay)
    style = object.__new__(P.StyleGuidanceOperator)                                   # no tower is built: the type alone is refused
    with pytest.raises(ValueError, match="10-second"):
        P.TrackOperator(style, lay)
    with pytest.raises(ValueError, match="at most 64"):
        P.TrackOperator(_Inner(), P.TrackLayout(6400 + 65 * 4800, 6400, 1600))
    inner.noiser = None
    with pytest.raises(ValueError, match="6400 samples"):
        op.guidance(torch.zeros(3, 6432), 6000, None, "mel_spectrogram")
    with pytest.raises(ValueError, match="expected \\(3, >= 6400\\)"):
        op.stitch(torch.zeros(2, 6432))


def test_new_entry_points_are_bound_in_both_bindings():
    import os
    from diffmusic_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "diffmusic_hip.h")).read()
    src = open(os.path.join(root, "diffmusic_amd", "csrc_torch", "torch_ops.cpp")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib._SIGS and s in _lib.ADDED_IN_V4 and f"int {s}(" in hdr and f"#pragma weak {s}" in src
    assert "#define DMX_ABI_VERSION 4 " in hdr and _lib.ABI_VERSION == 4
    for name in NEW_OPS:
        assert name in ops.OP_NAMES and f'm.def("{name}(' in src
    h = ops.load()                                                                    # no CPU fallback, in either binding: a CPU tensor
    with pytest.raises(RuntimeError, match="on the GPU"):                             # is refused before anything is launched
        h.track_stitch_fwd(torch.zeros(1, 8), [0], 8, 4, 8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        h.track_stitch_bwd(torch.zeros(1, 8), [0], 8, 4, 8)
    with pytest.raises(RuntimeError, match="on the GPU"):
        ops.ctypes_hip.track_stitch_fwd(torch.zeros(1, 8), [0], 8, 4, 8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.ctypes_hip.track_stitch_bwd(torch.zeros(1, 8), [0], 8, 4, 8)


def test_scheduler_refuses_per_clip_norms_for_a_track():
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    from tests.stubs import SCHED
    op = P.TrackOperator(_Inner(), P.TrackLayout(16000, 6400, 1600))
    s = get_scheduler("dps")(operator=op, **SCHED)
    s.set_timesteps(10)
    x = torch.zeros(3, 8, 10, 16)
    with pytest.raises(ValueError, match="per_clip_norm=False"):
        s.step(x, s._timesteps_host[0], x)


# ---- the pipeline's track branch on the CPU stand-ins -----------------------------------------------------------------------------
N, SECONDS, L = 6, 0.64, 10240            # 0.64 s -> mel height 64 -> latent (W, 8, 16, 4), windows of 10240 samples


def _track_pipe(T=25600, R=2560, inner=None, per_clip_norm=False, **sched_kw):
    from diffmusic_amd import inverse_problem as P

    class CpuTrackOperator(P.TrackOperator):
        """The stitch launch replaced by its torch restatement; everything the pipeline checks is the product's."""

        def stitch(self, wav):
            lay = self.layout
            assert wav.shape[0] == lay.num_windows and wav.shape[1] >= lay.window_len
            wt = torch.from_numpy(weights64(lay))
            out = torch.zeros(lay.track_len, dtype=torch.float64)
            for w, s in enumerate(lay.starts):
                out[s:s + lay.window_len] += wt[w, s:s + lay.window_len] * wav[w, :lay.window_len].double()
            return out.float()[None]

    pipe = make_pipeline(per_clip_norm=per_clip_norm, **sched_kw)
    lay = P.TrackLayout(T, L, R)
    pipe.scheduler.operator = CpuTrackOperator(inner if inner is not None else _Inner(), lay)
    return pipe, lay


def _call(pipe, W, **kw):
    pe = torch.randn(W, 512, generator=torch.Generator().manual_seed(99))
    args = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N, show_progress=False, eta=0.0,
                generator=[torch.Generator().manual_seed(s) for s in range(W)])
    args.update(kw)
    return pipe(**args)


def test_pipeline_returns_the_stitched_track():
    pipe, lay = _track_pipe()
    assert lay.num_windows == 3
    out = _call(pipe, 3)
    assert out.audios.shape == (1, lay.track_len) and out.audios.dtype == np.float32 and np.isfinite(out.audios).all()
    assert len(pipe.last_losses) == N and pipe.scheduler.operator.inner.resets >= 1
    lat = _call(pipe, 3, output_type="latent").audios
    assert lat.shape == (3, 8, 16, 4)                                                 # the W latents, not a track
    # the returned track is S applied to the windows an ordinary call on the same latents decodes
    plain = make_pipeline(per_clip_norm=False)
    wins = _call(plain, 3).audios
    assert wins.shape == (3, L)
    want = pipe.scheduler.operator.stitch(torch.from_numpy(wins)).numpy()
    assert np.array_equal(out.audios, want)
    single = lay.starts[1] - 1                                                        # covered by window 0 alone
    assert out.audios[0, single] == wins[0, single] and out.audios[0, -1] == wins[2, -1]
    t = _call(pipe, 3, output_type="pt", return_dict=False)[0]
    assert isinstance(t, torch.Tensor) and t.shape == (1, lay.track_len)


def test_pipeline_track_refusals():
    from diffmusic_amd import inverse_problem as P
    pipe, lay = _track_pipe()
    with pytest.raises(ValueError, match="3 windows"):
        _call(pipe, 2)                                                                # window count
    with pytest.raises(ValueError, match="window_len"):
        _call(pipe, 3, audio_length_in_s=0.32)                                        # window length
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
    clipnorm, _ = _track_pipe(per_clip_norm=True)
    with pytest.raises(ValueError, match="per_clip_norm=False"):
        _call(clipnorm, 3)
    noisy, _ = _track_pipe()
    noisy.scheduler.operator.inner.noiser = P.GaussianNoise(0.05, stream="clip")
    with pytest.raises(ValueError, match="global noise stream"):
        _call(noisy, 3)
    noisy.scheduler.operator.inner.noiser = P.GaussianNoise(0.05, stream="global")    # the global stream is allowed
    assert _call(noisy, 3).audios.shape == (1, lay.track_len)
    one, lay1 = _track_pipe(T=L)                                                      # T == L: one window, still a (1, T) track
    assert lay1.num_windows == 1 and _call(one, 1).audios.shape == (1, L)
    assert pipe.scheduler.calls == 0                                                  # every refusal came before the first step


def test_a_call_without_a_track_operator_never_reaches_the_track_branch(monkeypatch):
    """A plain operator (or none) on the scheduler: neither the track checks nor a stitch run, and the clips come back as clips."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.pipelines.pipeline_musicldm import MusicLDMPipeline
    reached = []
    monkeypatch.setattr(MusicLDMPipeline, "_check_track", lambda self, *a, **k: reached.append("check"))
    monkeypatch.setattr(P.TrackOperator, "stitch", lambda self, wav: reached.append("stitch"))
    for op in (None, _Inner()):
        pipe = make_pipeline(per_clip_norm=False)
        pipe.scheduler.operator = op
        assert _call(pipe, 3).audios.shape == (3, L)
    assert reached == []
