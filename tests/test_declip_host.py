"""CPU: the host side of declipping -- `threshold_for_sdr`, the DeclippingOperator's refusals (it is built without a GPU: front end and
device thresholds are made on first use), the example's task wiring and the C-ABI bookkeeping of the new entry points."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEN = 6400


def _signal():
    """The two-clip test signal of tests/test_gpu_step.py."""
    g = torch.Generator().manual_seed(77)
    return 0.3 * torch.sin(torch.arange(LEN) * 0.05)[None] * torch.tensor([[1.0], [0.6]]) + 0.05 * torch.randn(2, LEN, generator=g)


def _sdr_db(x, c):
    x = np.asarray(x, dtype=np.float64)
    r = x - np.clip(x, -c, c)
    return 10.0 * np.log10(np.dot(x, x) / np.dot(r, r))


def test_sdr_formula_on_fixed_thresholds():
    """Orientation figures of the signal: thresholds 0.05 / 0.1 / 0.2 give 1.9 / 4.2 / 10.6 dB on clip 0 with 89 / 78 / 52 % clipped."""
    x = _signal()[0].double().numpy()
    for c, db, share in ((0.05, 1.9, 0.89), (0.1, 4.2, 0.78), (0.2, 10.6, 0.52)):
        assert abs(_sdr_db(x, c) - db) < 0.051, (c, _sdr_db(x, c))
        assert abs(float((np.abs(x) > c).mean()) - share) < 0.0051, c


@pytest.mark.parametrize("target", [3.0, 10.0])
def test_threshold_for_sdr_hits_the_asked_sdr(target):
    from diffmusic_amd.inverse_problem import threshold_for_sdr
    clean = _signal()
    c = threshold_for_sdr(clean, target)
    assert c.shape == (2,) and c.dtype == np.float64 and bool((c > 0).all())
    for b in range(2):
        got = _sdr_db(clean[b].double().numpy(), c[b])
        assert abs(got - target) < 1e-6, (b, got)
    assert c[1] < c[0]                                       # the quieter clip clips lower for the same SDR
    one = threshold_for_sdr(clean[0], target)                # a single (L,) clip
    assert one.shape == (1,) and one[0] == c[0]
    assert np.array_equal(threshold_for_sdr(clean.numpy(), target), c)


def test_threshold_for_sdr_refusals():
    from diffmusic_amd.inverse_problem import threshold_for_sdr
    clean = _signal()
    for bad in (0.0, -3.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sdr_db"):
            threshold_for_sdr(clean, bad)
    with pytest.raises(ValueError, match="all zero"):
        threshold_for_sdr(torch.stack([clean[0], torch.zeros(LEN)]), 3.0)


def test_constructor_and_batch_refusals():
    from diffmusic_amd import inverse_problem as P
    for bad in (0.0, -0.1, [0.1, 0.0], torch.tensor([0.2, -1.0]), float("nan"), []):
        with pytest.raises(ValueError, match="threshold"):
            P.DeclippingOperator(16000, bad)
    op = P.DeclippingOperator(16000, [0.1, 0.2])             # builds without a GPU
    assert op.per_clip and op.threshold.dtype == torch.float32 and op.threshold.tolist() == pytest.approx([0.1, 0.2])
    with pytest.raises(ValueError, match="2 per-clip"):
        op.forward(torch.zeros(3, 100))
    with pytest.raises(ValueError, match="2 per-clip"):
        op.guidance(torch.zeros(3, 100), 100, torch.zeros(3, 100), "mel_spectrogram")
    with pytest.raises(ValueError, match="2 per-clip"):
        op.thresholds(1, torch.device("cpu"))
    assert op.thresholds(2, torch.device("cpu")).tolist() == pytest.approx([0.1, 0.2])
    scalar = P.DeclippingOperator(16000, 0.25)               # a scalar broadcasts over any batch
    assert not scalar.per_clip
    assert scalar.thresholds(3, torch.device("cpu")).tolist() == [0.25] * 3 and scalar.thresholds(1, torch.device("cpu")).tolist() == [0.25]
    assert not P.DeclippingOperator(16000, torch.tensor(0.25)).per_clip and not P.DeclippingOperator(16000, np.float32(0.25)).per_clip
    with pytest.raises(RuntimeError, match="GPU only"):      # no CPU fallback
        scalar.forward(torch.zeros(2, 100))


def test_project_is_refused_under_measurement_noise():
    from diffmusic_amd import inverse_problem as P
    op = P.DeclippingOperator(16000, 0.1, noiser=P.GaussianNoise(0.05))
    with pytest.raises(ValueError, match="sigma > 0"):
        op.project(torch.zeros(1, 100), torch.zeros(1, 100))
    quiet = P.DeclippingOperator(16000, 0.1, noiser=P.GaussianNoise(0.0))
    with pytest.raises(RuntimeError, match="GPU only"):      # past the refusal: the projection itself needs the GPU
        quiet.project(torch.zeros(1, 100), torch.zeros(1, 100))


def _example():
    spec = importlib.util.spec_from_file_location("run_inverse_problem", os.path.join(ROOT, "examples", "run_inverse_problem.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_builds_the_declipping_operator():
    from diffmusic_amd import constants, inverse_problem as P
    from diffmusic_amd.config import compose
    mod = _example()
    assert constants.MUSIC_DECLIPPING == "music_declipping" and "music_declipping" in mod.TASKS
    cfg = compose("dps", overrides=["data=moises", "model=musicldm", "inverse_problem=music_declipping"])
    assert cfg.inverse_problem.name == "music_declipping" and cfg.inverse_problem.noise.sigma == 0.0
    thr = P.threshold_for_sdr(_signal(), 3.0)
    op, scale = mod.build_operator("music_declipping", cfg, "box", clip_threshold=thr)
    assert isinstance(op, P.DeclippingOperator) and scale == 1 and op.per_clip
    assert op.threshold.tolist() == pytest.approx(thr.tolist(), rel=1e-6) and op.noiser.additive_sigma == 0.0
    with pytest.raises(ValueError, match="clip_threshold"):
        mod.build_operator("music_declipping", cfg, "box")
    args = mod.parse_args(["-t", "music_declipping", "--project", "--init", "measurement", "--strength", "0.5"])
    assert args.clip_sdr_db == 3.0 and args.project and "music_declipping" not in mod.NO_WARM_START
    y = torch.zeros(2, LEN)
    assert mod.init_from_measurement("music_declipping", y, LEN) is y          # a clipped take is a natural init_audio


def test_new_entry_points_are_additive():
    """ABI version 4 stays; the new symbols are declared, bound, weak in the op library and checked by name at load."""
    from diffmusic_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "diffmusic_hip.h")).read()
    src = open(os.path.join(ROOT, "diffmusic_amd", "csrc_torch", "torch_ops.cpp")).read()
    assert "#define DMX_ABI_VERSION 4 " in hdr and _lib.ABI_VERSION == 4
    for s in ("dmx_audio_guidance_fwd_shaped", "dmx_audio_guidance_bwd_shaped", "dmx_clip_fwd", "dmx_clip_bwd", "dmx_declip_project"):
        assert s in _lib._SIGS and s in _lib.ADDED_IN_V4 and f"int {s}(" in hdr and f"#pragma weak {s}" in src, s
    for name in ("mel_guidance", "clip_fwd", "clip_bwd", "declip_project"):
        assert name in ops.OP_NAMES and f'm.def("{name}(' in src, name
    from diffmusic_amd.build import build_torch_ops
    assert os.path.exists(build_torch_ops())
    assert [a.name for a in ops.load().mel_guidance.default._schema.arguments][-4:] == ["noise", "noise_mag", "sigma", "thr"]
