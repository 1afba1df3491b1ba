"""CPU: the float64 model, the code rule, the element-wise bound, the fp32 emulation and the mutants of the MDCT quantiser
(tests/mdct_cases.py), the host helpers of inverse_problem/dsp.py, the CodecOperator's constructor, refusals and dead span, a torch
restatement of A with the straight-through backward (`CodecSTE`, which tests/test_gpu_codec.py imports) and the example's argument rules.
The GPU side (tests/test_gpu_codec.py) compares the kernel with the same model under the same rule and bound."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import mdct_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- a torch restatement of A = Phi^T Q Phi with the straight-through backward Phi^T K Phi (any device, any float dtype)
def _torch_basis(ref):
    return torch.from_numpy(M.basis() * M.window()[:, None]).to(device=ref.device, dtype=ref.dtype)          # (1024, 512), windowed


def torch_mdct(x):
    """x (B, L) -> (B, T, 512)"""
    L = x.shape[-1]
    T = M.frames(L)
    pad = torch.nn.functional.pad(x, (M.N, (T + 1) * M.N - M.N - L))
    return pad.unfold(-1, M.NF, M.N) @ _torch_basis(x)


def torch_imdct(C, L):
    """C (B, T, 512) -> (B, L), the transpose of `torch_mdct`"""
    B, T = C.shape[0], C.shape[1]
    fr = C @ _torch_basis(C).T
    out = torch.zeros(B, (T + 1) * M.N, dtype=C.dtype, device=C.device)
    out[:, :T * M.N] += fr[..., :M.N].reshape(B, -1)
    out[:, M.N:] += fr[..., M.N:].reshape(B, -1)
    return out[:, M.N:M.N + L]


def torch_quantise(C, D):
    """C (B, T, 512), D broadcastable (.., T, 512) -> Q(C): rint half-even (torch.round), D = 0 transparent, D = inf discards"""
    D = D.to(C.dtype).expand_as(C)
    coded = (D > 0) & torch.isfinite(D)
    q = C / torch.where(coded, D, torch.ones_like(D))
    coded = coded & (q.abs() < M.Q_LIMIT)
    return torch.where(coded, torch.round(q) * torch.where(coded, D, torch.zeros_like(D)), torch.where(torch.isinf(D), torch.zeros_like(C), C))


class CodecSTE(torch.autograd.Function):
    """y = Phi^T Q(Phi x) for x (B, L) and steps D_t (T, 512) or (B, T, 512) -- the kernel's layout; backward: the straight-through rule
    dx = Phi^T K Phi dy, K = [D < inf]"""

    @staticmethod
    def forward(ctx, x, D_t):
        ctx.save_for_backward(D_t)
        return torch_imdct(torch_quantise(torch_mdct(x), D_t), x.shape[-1])

    @staticmethod
    def backward(ctx, dy):
        (D_t,) = ctx.saved_tensors
        C = torch_mdct(dy)
        keep = (~torch.isinf(D_t)).to(C.dtype).expand_as(C)
        return torch_imdct(C * keep, dy.shape[-1]), None


# ---- the model, the bound, the emulation, the mutants
@pytest.mark.parametrize("c", M.CASES, ids=lambda c: c.name)
def test_emulation_obeys_the_code_rule_and_lies_within_the_bound_in_every_element(c):
    for mode in M.MODES:
        r, broken, differing = M.run_case(c, mode)
        print(f"{c.name} {mode}: largest |emulation - model| / bound = {r:.4f}; codes off the rule {broken}, ambiguous and differing {differing}")
        assert broken == 0 and r <= 1.0, (c.name, mode, r, broken)


@pytest.mark.parametrize("name", sorted(M.MUTANTS))
def test_every_mutant_leaves_the_bound_or_changes_a_code(name):
    where, mode, cases = M.MUTANTS[name]
    res = {cn: M.run_case(M.CASE[cn], mode, name, where) for cn in cases}
    print(name, res)
    assert any(r > 1.0 or broken > 0 for r, broken, _ in res.values()), (name, res)


@pytest.mark.parametrize("c", M.CASES, ids=lambda c: c.name)
def test_ambiguous_share_stays_under_the_cap(c):
    amb = M.reference(c).amb
    print(f"{c.name}: {int(amb.sum())} of {amb.size} coefficients ambiguous ({100.0 * amb.mean():.3f} %)")
    assert amb.mean() <= M.AMBIG_CAP
    if c.name in M.STEP_CASES:
        assert not amb.any()


def test_case_table_covers_the_branches():
    assert {300, 512, 513, 1024, 4096, 4097, 4999, 6400} <= {c.L for c in M.CASES}
    assert M.SLAB == 4096 and M.frames(300) == 2 and M.frames(512) == 2 and M.frames(513) == 3 and M.frames(6400) == 14
    assert all(c.B == 2 and c.why for c in M.CASES)
    for L in (300, 512, 513, 1024, 4096, 4097, 4999, 6400):
        kinds = {(c.step, c.per_clip) for c in M.CASES if c.L == L}
        assert {("zero", False), ("rand", False), ("rand", True)} <= kinds, L
    steps = {c.step for c in M.CASES}
    for s in ("lowpass", "coef0", "coef1", "coef510", "coef511", "frame_first", "frame_last", "frame_edge", "dead_frames"):
        assert s in steps, s
    assert any(c.stride == 6432 and c.L == 6400 and c.full > c.L for c in M.CASES)
    i = M.inputs(M.CASE["L4999_edge"])
    assert np.signbit(i.x[0, 17]) and i.x[0, 17] == 0 and np.abs(i.x).max() >= 1e3
    assert set(M.STEP_CASES) <= set(M.CASE) and all(M.CASE[n].L == 6400 for n in M.STEP_CASES)


@pytest.mark.parametrize("L", [300, 512, 513, 1024, 4097, 4999, 6400])
def test_model_reconstructs_the_clip_and_keeps_its_energy(L):
    x = np.random.default_rng(L).standard_normal((2, L))
    r = M.analysis(x, L)
    y = M.synthesis(r, r.C).y
    assert np.abs(y - x).max() <= 1e-12
    assert np.abs((r.C ** 2).sum((1, 2)) / (x ** 2).sum(1) - 1.0).max() <= 1e-12
    assert np.abs(M.analysis_fft(x, L) - r.C).max() <= 1e-12                 # the kernel's FFT route is the definition
    z = M.synthesis(r, r.C)
    pre = np.exp(-1j * np.pi * np.arange(M.NF) / M.NF)
    assert np.abs((z.z * np.conj(pre)).real * math.sqrt(2.0 / M.N) - z.g).max() <= 1e-12    # and so is the transpose's


def test_window_is_princen_bradley():
    w = M.window()
    assert np.abs(w[:M.N] ** 2 + w[M.N:] ** 2 - 1.0).max() < 1e-14


@pytest.mark.parametrize("L,per_clip", [(300, False), (4097, True), (4999, False)])
def test_pass_is_symmetric(L, per_clip):
    rng = np.random.default_rng(L + 1)
    x, y = rng.standard_normal((2, L)), rng.standard_normal((2, L))
    D = rng.uniform(0.0, 1.0, ((2,) if per_clip else ()) + (M.N, M.frames(L)))
    D[..., 200:, :] = np.inf
    D[..., 3, 1] = np.inf
    Ax, Ay = M.expect(x, D, L, M.PASS)[0], M.expect(y, D, L, M.PASS)[0]
    for b in range(2):
        lhs, rhs = float(Ax[b] @ y[b]), float(x[b] @ Ay[b])
        scale = float(np.abs(Ax[b]) @ np.abs(y[b]) + np.abs(x[b]) @ np.abs(Ay[b]))
        assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)


@pytest.mark.parametrize("step", [0.01, 0.05, 0.2, 1.0])
def test_recoding_the_measurement_gives_the_codecs_own_codes_on_whole_frames(step):
    c = M.CASE["L6400_rand"]
    x = M.inputs(c).x.astype(np.float64)
    D = np.full((2, c.T, M.N), step)
    r = M.analysis(x, c.L)
    q, f = M.quantise(r.C, D)
    y = M.synthesis(r, f).y
    q2, _ = M.quantise(M.analysis(y, c.L).C, D)
    whole = M.whole_frames(c.L, c.T)
    assert whole.sum() == c.T - 3 and (q2[:, whole] == q[:, whole]).all()    # L = 6400: frames 1 .. 11 of 0 .. 13
    assert (q2[:, ~whole] != q[:, ~whole]).any()                              # the edge frames are not whole: their codes differ


def test_project_properties_in_the_model():
    c = M.CASE["L6400_rand"]
    i, ref = M.inputs(c), M.reference(c)
    x = i.x.astype(np.float64)
    whole = M.whole_frames(c.L, c.T)
    _, f = M.quantise(ref.r.C, ref.D)
    y = M.synthesis(ref.r, f).y                                               # the measurement
    qy, _ = M.quantise(M.analysis(y, c.L).C, ref.D)
    # a consistent signal (the clean clip, whose codes are the measurement's): whole frames are left alone
    Cx = ref.r.C
    Px = M.projected(Cx, ref.D, qy, c.L)
    assert np.abs(Px - Cx)[:, whole].max() <= 1e-12
    # an inconsistent one (another clip) is moved into the cells on whole frames, and only there
    Co = M.analysis(i.other, c.L).C
    Po = M.projected(Co, ref.D, qy, c.L)
    lo, hi, active = M.cells(ref.D, qy, c.L)
    assert active[:, whole].all() and not active[:, ~whole].any()
    assert ((Po >= lo) & (Po <= hi))[active].all() and (np.abs(Po - Co)[active] > 0).mean() > 0.5
    assert (Po[:, ~whole] == Co[:, ~whole]).all()
    # transparent, discarded and uncoded coefficients stay
    D2 = ref.D.copy()
    D2[:, :, :10], D2[:, :, 300:] = 0.0, np.inf
    q2, _ = M.quantise(Cx, D2)
    P2 = M.projected(Co, D2, q2, c.L)
    assert (P2[:, :, :10] == Co[:, :, :10]).all() and (P2[:, :, 300:] == Co[:, :, 300:]).all()


def test_the_planted_tie_rounds_half_to_even_in_the_emulation():
    c = M.CASE["L6400_rand"]
    C = M.emulate_coeffs(M.inputs(c).x, c.L)
    for half, want in ((2.5, 2), (3.5, 4), (0.5, 0), (1.5, 2)):
        ties = M.plant_tie(C, half)
        assert len(ties) >= 8, (half, len(ties))
        D = np.ones(C.shape, np.float32)
        for idx, d in ties:
            D.reshape(-1)[idx] = d
        codes, _ = M.emulate_quantise(C, D)
        trunc, _ = M.emulate_quantise(C, D, mut="truncation")
        for idx, _ in ties:
            s = int(np.sign(C.reshape(-1)[idx]))
            assert int(codes.reshape(-1)[idx]) == s * want, (half, idx)
        if want != math.floor(half):                                       # 1.5 and 3.5 round up: truncation shows there
            assert all(int(trunc.reshape(-1)[idx]) != int(codes.reshape(-1)[idx]) for idx, _ in ties)
    q, _ = M.quantise(np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5]), np.ones(6))    # the float64 model rounds the same way
    assert q.tolist() == [0, 2, 2, 0, -2, -2]


def test_quantiser_special_steps_in_the_model():
    C = np.array([0.3, -0.7, 1e9, 0.26, -0.26, np.nan])
    q, f = M.quantise(C, np.array([0.0, np.inf, 1.0, 0.5, 0.5, 0.5]))
    assert q.tolist() == [M.MARK, 0, M.MARK, 1, -1, M.MARK]
    assert f[:5].tolist() == [0.3, 0.0, 1e9, 0.5, -0.5] and np.isnan(f[5])
    assert M.MARK == -2 ** 31


def test_dead_samples_are_exactly_zero_in_the_model_and_their_bound_is_zero():
    c = M.CASE["L6400_dead_frames"]
    i = M.inputs(c)
    for mode in (M.QUANT, M.PASS):
        y, b = M.expect(i.x, i.step, c.L, mode)
        assert (y[:, 3072:6144] == 0).all() and (b[:, 3072:6144] == 0).all()      # frames 6 .. 12 -> [512 * 6, 512 * 12)
        assert (y[:, 3071] != 0).all() and (y[:, 6144] != 0).all()
    e, _ = M.emulate(i.x, i.step, c.L, M.QUANT)
    z = e[:, 3072:6144]
    assert (z == 0).all() and not np.signbit(z).any()


# ---- host helpers (inverse_problem/dsp.py)
def test_mdct_frames_and_transforms_are_the_models():
    from diffmusic_amd.inverse_problem import mdct_frames, mdct, imdct
    assert [mdct_frames(L) for L in (1, 300, 512, 513, 1024, 6400, 160000)] == [2, 2, 2, 3, 3, 14, 314]
    with pytest.raises(ValueError):
        mdct_frames(0)
    for L in (300, 513, 4999):
        x = np.random.default_rng(L).standard_normal((2, L))
        C = mdct(x)
        assert C.shape == (2, 512, mdct_frames(L))
        assert np.abs(C - M.analysis(x, L).C.transpose(0, 2, 1)).max() <= 1e-12
        assert np.abs(imdct(C, L) - x).max() <= 1e-12
        assert np.abs(mdct(x[0]) - C[0]).max() == 0
    with pytest.raises(ValueError, match="512"):
        imdct(np.zeros((512, 5)), 300)


def test_codec_bands_and_step_grid():
    from diffmusic_amd.inverse_problem import codec_bands, codec_step_grid
    e = codec_bands(16000)
    assert e.shape == (22,) and e[0] == 0 and e[-1] == 512 and (np.diff(e) >= 1).all()
    w = np.diff(e)
    assert w[0] <= w[-1] and w[:8].max() <= w[-4:].min()                   # Bark-like: narrow at the bottom, wide at the top
    assert (np.diff(codec_bands(16000, 512)) == 1).all()
    with pytest.raises(ValueError):
        codec_bands(16000, 0)
    g = codec_step_grid(6400, 16000, -40.0)
    assert g.shape == (512, 14) and g.dtype == np.float32 and np.allclose(g, 0.01) and (g == g[:, :1]).all()
    g = codec_step_grid(6400, 16000, -40.0, cutoff_hz=4000.0)             # centres (k + 1/2) 15.625 Hz: k = 255 at 3992.2, k = 256 at 4007.8
    assert np.isinf(g[256:]).all() and np.isfinite(g[:256]).all()
    g = codec_step_grid(6400, 16000, -40.0, tilt_db_per_octave=6.0)
    k1, k2 = 63, 127                                                      # 992.2 Hz and 1992.2 Hz: about one octave
    assert abs(20 * math.log10(g[k2, 0] / g[k1, 0]) - 6.0 * math.log2(127.5 / 63.5)) < 1e-4
    for bad in (dict(step_db=math.nan), dict(step_db=-40.0, cutoff_hz=-1.0), dict(step_db=-40.0, tilt_db_per_octave=math.inf)):
        with pytest.raises(ValueError):
            codec_step_grid(6400, 16000, **bad)


@pytest.mark.parametrize("nmr_db", [10.0, 20.0])
def test_codec_steps_for_nmr_reaches_its_noise_to_mask_ratio_within_1_db(nmr_db):
    from diffmusic_amd.inverse_problem import codec_steps_for_nmr, codec_bands
    L, sr = 6400, 16000
    rng = np.random.default_rng(7)
    X = np.fft.rfft(rng.standard_normal((2, L)))
    X[:, int(3500 * L / sr):] = 0                                          # band-limited to 3.5 kHz
    x = 0.3 * np.fft.irfft(X, n=L) + 0.1 * np.sin(2 * np.pi * 440.0 / sr * np.arange(L))
    D = codec_steps_for_nmr(x, sr, nmr_db, cutoff_hz=3500.0)
    assert D.shape == (2, 512, M.frames(L)) and D.dtype == np.float32 and np.isinf(D[:, 224:]).all() and np.isfinite(D[:, :224]).all()
    assert codec_steps_for_nmr(x[0], sr, nmr_db).shape == (512, M.frames(L))
    r = M.analysis(x, L)
    Db = M.step_btk(D, 2)
    _, f = M.quantise(r.C, Db)
    whole = M.whole_frames(L, M.frames(L))
    e = codec_bands(sr)
    sig = noise = 0.0
    for lo, hi in zip(e[:-1], e[1:]):
        if hi <= 224:
            sig += (r.C[:, whole, lo:hi] ** 2).sum()
            noise += ((f - r.C)[:, whole, lo:hi] ** 2).sum()
    got = 10 * math.log10(sig / noise)
    print(f"nmr_db {nmr_db}: measured {got:.2f} dB")
    assert abs(got - nmr_db) <= 1.0
    with pytest.raises(ValueError):
        codec_steps_for_nmr(x, sr, math.nan)
    with pytest.raises(ValueError):
        codec_steps_for_nmr(np.zeros((2, 2, 8)), sr, 10.0)


# ---- the operator without a GPU
def _op(step, **kw):
    from diffmusic_amd.inverse_problem import CodecOperator
    return CodecOperator(16000, step, **kw)


def test_constructor_refusals_need_no_gpu():
    T = 14
    op = _op(np.full((512, T), 0.1, np.float32))
    assert not op.per_clip and op.step_frames == T and op.frames(6400) == T and op.dead_span(6400) is None and op.lossless
    assert op.positional_state is None and op._on_load(None, 6400) is None
    pc = _op(torch.full((3, 512, T), 0.1))
    assert pc.per_clip and pc.positional_state == ("CodecOperator with per-clip step grids", "step grids")
    for bad in (np.ones(512), np.ones((513, T)), np.ones((2, 2, 512, T)), np.ones((T, 512))):
        with pytest.raises(ValueError, match="512"):
            _op(bad)
    with pytest.raises(ValueError, match="step"):
        _op(None)
    for v in (math.nan, -1e-3, -math.inf):
        g = np.ones((512, T), np.float32)
        g[5, 5] = v
        with pytest.raises(ValueError, match="negative or NaN"):
            _op(g)
    g = np.ones((512, T), np.float32)
    g[5, 5], g[6, 6] = math.inf, 0.0                                       # both ends of [0, +inf] are steps
    assert not _op(g).lossless


def test_shape_errors_name_the_expected_shape_before_any_gpu_work():
    op = _op(np.ones((512, 14), np.float32))
    x = torch.zeros(2, 6657)                                              # T would be 15
    for call in (lambda: op.forward(x), lambda: op.apply(x, 6657), lambda: op.guidance(x, 6657, x, "wav_form")):
        with pytest.raises(ValueError, match=r"\(512, 15\)"):
            call()
    op = _op(np.ones((3, 512, 14), np.float32))
    x = torch.zeros(2, 6400)
    for call in (lambda: op.forward(x), lambda: op.apply(x, 6400), lambda: op.guidance(x, 6400, x, "mel_spectrogram")):
        with pytest.raises(ValueError, match=r"\(2, 512, 14\)"):
            call()


def test_project_refuses_measurement_noise_by_name():
    from diffmusic_amd.inverse_problem import GaussianNoise
    op = _op(np.ones((512, 14), np.float32), noiser=GaussianNoise(0.01))
    with pytest.raises(ValueError, match="sigma > 0"):
        op.project(torch.zeros(1, 6400), torch.zeros(1, 6400))


def test_dead_span_on_hand_made_grids():
    T, L = 14, 6400
    g = np.full((512, T), 0.1, np.float32)
    g[:, 5] = np.inf                                          # one discarded frame: every sample still has its other frame
    assert _op(g).dead_span(L) is None
    g[:, 5:7] = np.inf                                        # frames 5, 6: the hop both cover, [512 * 5, 512 * 6)
    assert _op(g).dead_span(L) == (2560, 3072)
    g[:, 8:13] = np.inf                                       # the longest run wins: frames 8 .. 12 -> [4096, 6144)
    assert _op(g).dead_span(L) == (4096, 6144)
    assert _op(g).dead_span(L + 512) is None                  # another clip length: no claim
    g[100, 10] = 1e30                                         # one kept coefficient splits the run: 8 .. 9 and 11 .. 12
    assert _op(g).dead_span(L) == (2560, 3072)
    pc = np.stack([g, g])
    pc[1, :, 5:7] = 0.1                                       # every clip has to be discarded there
    assert _op(pc).dead_span(L) == (4096, 4608)
    g = np.full((512, T), 0.1, np.float32)
    g[:, 10:] = np.inf                                        # up to the last frame: the span ends with the clip
    assert _op(g).dead_span(L) == (5120, 6400)
    g = np.full((512, T), np.inf, np.float32)
    assert _op(g).dead_span(L) == (0, 6400)
    c = M.CASE["L6400_dead_frames"]
    assert _op(M.inputs(c).step).dead_span(6400) == (3072, 6144)


def test_pipeline_refuses_lanes_and_shards_for_per_clip_grids_only():
    from diffmusic_amd.pipelines.pipeline_musicldm import MusicLDMPipeline
    from types import SimpleNamespace

    def check(op, **kw):
        pipe = SimpleNamespace(scheduler=SimpleNamespace(operator=op), lanes=1)
        return MusicLDMPipeline._check_positional_state(pipe, kw.get("shard", False), kw.get("group"), kw.get("lanes"))
    shared, per_clip = _op(np.ones((512, 14), np.float32)), _op(np.ones((2, 512, 14), np.float32))
    check(shared, lanes=2)
    check(shared, shard=True)
    check(per_clip)
    with pytest.raises(ValueError, match="lanes.*step grids|step grids.*lanes"):
        check(per_clip, lanes=2)
    with pytest.raises(ValueError, match="shard"):
        check(per_clip, shard=True)


# ---- the torch restatement
@pytest.mark.parametrize("name", ["L6400_coarse_lowpass", "L4999_rand_pc", "L300_zero"])
def test_restatement_is_the_model_and_its_backward_is_the_pass_model(name):
    c = M.CASE[name]
    i = M.inputs(c)
    x = torch.from_numpy(i.x.astype(np.float64)).requires_grad_(True)
    D_t = torch.from_numpy(np.ascontiguousarray(np.swapaxes(i.step, -1, -2)))
    y = CodecSTE.apply(x, D_t)
    want, _ = M.expect(i.x, i.step, c.L, M.QUANT)
    assert np.abs(y.detach().numpy() - want).max() <= 1e-10
    dy = torch.from_numpy(i.other.astype(np.float64))
    (g,) = torch.autograd.grad(y, x, dy)
    assert np.abs(g.numpy() - M.expect(i.other, i.step, c.L, M.PASS)[0]).max() <= 1e-10
    if not np.isinf(i.step).any():
        assert np.abs(g.numpy() - i.other).max() <= 1e-10                 # no infinite step: the identity


# ---- examples/run_inverse_problem.py
def _example():
    spec = importlib.util.spec_from_file_location("run_inverse_problem", os.path.join(ROOT, "examples", "run_inverse_problem.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_argument_rules_and_operator():
    from diffmusic_amd.config import compose
    from diffmusic_amd import constants, inverse_problem as P
    mod = _example()
    assert constants.MUSIC_CODEC_RESTORATION == mod.CODEC == "music_codec_restoration" and mod.CODEC in mod.TASKS
    cfg = compose("dps", overrides=["data=moises", "model=musicldm", f"inverse_problem={mod.CODEC}"])
    assert cfg.inverse_problem.noise.name == "gaussian" and float(cfg.inverse_problem.noise.sigma) == 0.0
    t = ("-t", mod.CODEC)

    def params(*argv):
        return mod.codec_params(mod.parse_args(list(argv)), cfg)
    assert params(*t) == dict(nmr_db=12.0, cutoff_hz=6000.0, tilt_db_per_octave=0.0)             # nothing given: the yaml
    assert params(*t, "--codec_nmr_db", "6") == dict(nmr_db=6.0, cutoff_hz=6000.0, tilt_db_per_octave=0.0)
    assert params(*t, "--codec_step_db", "-30", "--codec_cutoff_hz", "4000") == dict(step_db=-30.0, cutoff_hz=4000.0, tilt_db_per_octave=0.0)
    assert params(*t, "--codec_cutoff_hz", "0")["cutoff_hz"] is None
    for bad in (("--codec_nmr_db", "6", "--codec_step_db", "-30"), ("--codec_nmr_db", "nan"), ("--codec_step_db", "1e9")):
        with pytest.raises(SystemExit):
            params(*t, *bad)
    for other in ("music_inpainting", "music_declipping"):
        assert mod.codec_params(mod.parse_args(["-t", other]), cfg) is None
        for flag in ("--codec_nmr_db", "--codec_step_db", "--codec_cutoff_hz"):
            with pytest.raises(SystemExit, match=mod.CODEC):
                mod.codec_params(mod.parse_args(["-t", other, flag, "3"]), cfg)
    sr = cfg.data.sample_rate
    L = int(cfg.model.pipe.audio_length_in_s * sr)
    op, scale = mod.build_operator(mod.CODEC, cfg, "box", codec=params(*t, "--codec_step_db", "-30"))
    assert isinstance(op, P.CodecOperator) and scale == 1 and tuple(op.step.shape) == (512, P.mdct_frames(L)) and not op.lossless
    assert torch.equal(op.step, torch.from_numpy(P.codec_step_grid(L, sr, -30.0, cutoff_hz=6000.0)))
    clean = 0.1 * torch.randn(2, 3000, generator=torch.Generator().manual_seed(0))
    op, _ = mod.build_operator(mod.CODEC, cfg, "box", codec=params(*t), codec_audio=clean)     # signal-adaptive: one grid per clip
    assert tuple(op.step.shape) == (2, 512, P.mdct_frames(3000)) and op.per_clip
    op, _ = mod.build_operator(mod.CODEC, cfg, "box", codec=params(*t), codec_audio=clean[0])  # a track: its one grid
    assert tuple(op.step.shape) == (512, P.mdct_frames(3000))
    with pytest.raises(ValueError, match="codec"):
        mod.build_operator(mod.CODEC, cfg, "box")
    with pytest.raises(ValueError, match="codec_audio"):
        mod.build_operator(mod.CODEC, cfg, "box", codec=params(*t))


def test_abi_surface_lists_the_new_entry_points():
    from diffmusic_amd import _lib, ops
    for name in ("dmx_mdct_frames", "dmx_mdct_quant", "dmx_mdct_project"):
        assert name in _lib._SIGS and name in _lib.ADDED_IN_V4
    assert _lib.ABI_VERSION == 4
    assert "mdct_quant" in ops.OP_NAMES and "mdct_project" in ops.OP_NAMES
    with pytest.raises((RuntimeError, AssertionError)):
        ops.ctypes_hip.mdct_quant(0, torch.zeros(1, 300), torch.ones(2, 512), 300, 300)          # no CPU fallback
