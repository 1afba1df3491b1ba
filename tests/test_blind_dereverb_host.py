"""CPU: the host side of blind dereverberation -- the operator's constructor rules (it is built without a GPU: front end and device state
are made on first use), the YAML, the example's task wiring, the pipeline's refusals and the C-ABI bookkeeping of the new entry points."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example():
    spec = importlib.util.spec_from_file_location("run_inverse_problem", os.path.join(ROOT, "examples", "run_inverse_problem.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_constructor_validation():
    from diffmusic_amd import inverse_problem as P
    op = P.BlindDereverberationOperator()
    assert (op.ir_length, op.decay_factor, op.lr, op.betas, op.adam_eps, op.k) == (800, 0.85, 0.05, (0.9, 0.999), 1e-8, 0)
    assert op.ir_estimate is None and op.true_ir is None and op.noiser is None
    for lr in (0, -0.1, float("nan"), float("inf"), "0.05"):
        with pytest.raises(ValueError, match="lr"):
            P.BlindDereverberationOperator(lr=lr)
    for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9,), (0.9, 0.999, 0.5), (0.9, float("nan"))):
        with pytest.raises(ValueError, match="betas"):
            P.BlindDereverberationOperator(betas=betas)
    with pytest.raises(ValueError, match="adam_eps"):
        P.BlindDereverberationOperator(adam_eps=-1e-8)
    for n in (0, 8193):
        with pytest.raises(ValueError, match="ir_length"):
            P.BlindDereverberationOperator(ir_length=n)
    for init in ("zeros", torch.zeros(799), torch.ones(2, 801), torch.ones(2, 3, 800), torch.zeros(800), torch.full((800,), float("nan"))):
        with pytest.raises(ValueError, match="init"):
            P.BlindDereverberationOperator(init=init)
    assert P.BlindDereverberationOperator(betas=(0.0, 0.0)).betas == (0.0, 0.0)


def test_initial_estimates():
    from diffmusic_amd import inverse_problem as P
    imp = P.BlindDereverberationOperator(ir_length=7)._start
    assert imp.shape == (1, 7) and imp[0].tolist() == [0, 0, 0, 1, 0, 0, 0]                # h[n // 2] = 1: A starts as the identity
    rows = torch.tensor([[0.5, -2.0, 1.0], [0.1, 0.2, 0.4]])
    op = P.BlindDereverberationOperator(ir_length=3, init=rows)
    assert torch.equal(op._start, torch.tensor([[0.25, -1.0, 0.5], [0.25, 0.5, 1.0]]))      # peak-normalised per row, sign kept
    assert rows[0, 1] == -2.0                                                              # the caller's tensor is not touched
    assert P.BlindDereverberationOperator(ir_length=3, init=rows[0])._start.shape == (1, 3)
    with pytest.raises(ValueError, match="2 response"):
        op._rows(op._start, 3, "init")                                                     # two rows cannot serve three clips
    ir = op.generate_impulse_response(50, 0.85)
    assert ir.shape == (1, 50) and float(ir.abs().max()) == 1.0
    with pytest.raises(RuntimeError, match="GPU only"):
        op.forward(torch.zeros(2, 100))
    assert op.true_ir.shape == (2, 3)                                                      # drawn once per clip before the launch is refused


def test_hooks_are_no_ops_on_the_other_operators():
    from diffmusic_amd import inverse_problem as P
    op = P.DeclippingOperator(16000, 0.1)
    assert op.after_cotangent(None, 0, None) is None and op.restart() is None
    assert op.after_cotangent(None, 0, None, ir=None, anything=1) is None
    lay = P.TrackLayout(11200, 6400, 1600)
    inner = P.BlindDereverberationOperator(ir_length=5)
    top = P.TrackOperator(inner, lay)
    inner.k = 3
    top.restart()
    assert inner.k == 0
    inner.k = 3
    top.reset_cache()
    assert inner.k == 0
    P.TrackOperator(op, lay).restart()                                                      # an inner operator without state


def test_yaml_composes_and_the_example_builds_the_operator():
    from diffmusic_amd import constants, inverse_problem as P
    from diffmusic_amd.config import compose
    mod = _example()
    assert constants.MUSIC_BLIND_DEREVERBERATION == "music_blind_dereverberation" and constants.MUSIC_BLIND_DEREVERBERATION in mod.TASKS
    cfg = compose("dps", overrides=["data=moises", "model=musicldm", "inverse_problem=music_blind_dereverberation"])
    assert cfg.inverse_problem.name == "music_blind_dereverberation" and cfg.inverse_problem.noise.sigma == 0.0
    assert cfg.inverse_problem.lr == 0.05
    cfg.inverse_problem["lr"] = 0.02
    op, scale = mod.build_operator("music_blind_dereverberation", cfg, "box")
    assert isinstance(op, P.BlindDereverberationOperator) and scale == 1
    assert (op.ir_length, op.decay_factor, op.lr) == (5000, 0.99, 0.02) and op.noiser.additive_sigma == 0.0
    plain = compose("dps", overrides=["data=moises", "model=musicldm"])                    # a config without `lr`: the default
    assert mod.build_operator("music_blind_dereverberation", plain, "box")[0].lr == 0.05
    args = mod.parse_args(["-t", "music_blind_dereverberation"])
    assert args.task == "music_blind_dereverberation" and "music_blind_dereverberation" not in mod.NO_WARM_START


def test_lanes_and_sharding_are_refused():
    from diffmusic_amd import inverse_problem as P
    from tests.stubs import make_pipeline
    pe = torch.nn.functional.normalize(torch.randn(2, 512, generator=torch.Generator().manual_seed(0)), dim=-1)
    call = dict(prompt_embeds=pe, audio_length_in_s=0.4, num_inference_steps=2, show_progress=False, measurement=torch.zeros(2, 6400))
    pipe = make_pipeline()
    pipe.scheduler.operator = P.BlindDereverberationOperator(ir_length=16)
    with pytest.raises(ValueError, match="lanes > 1"):
        pipe(lanes=2, **call)
    pipe.lanes = 2
    with pytest.raises(ValueError, match="lanes > 1"):
        pipe(**call)
    pipe.lanes = 1
    with pytest.raises(ValueError, match="sharded"):
        pipe(shard=True, **call)
    with pytest.raises(ValueError, match="sharded"):
        pipe(group=object(), **call)
    assert pipe.scheduler.calls == 0                                                       # refused before the first step
    out = pipe(output_type="latent", **call).audios                                       # one lane, one rank: the call runs
    assert out.shape[0] == 2 and pipe.scheduler.calls == 2
    pipe.scheduler.operator = None                                                         # any other operator: lanes as before
    assert pipe(lanes=2, output_type="latent", **call).audios.shape[0] == 2


def test_nan_retry_restarts_the_operator():
    from tests.stubs import make_pipeline
    pe = torch.nn.functional.normalize(torch.randn(2, 512, generator=torch.Generator().manual_seed(0)), dim=-1)
    pipe = make_pipeline(nan_at=(1,))
    log = []

    class Op:
        noiser = None

        def reset_cache(self):
            log.append("reset")

        def restart(self):
            log.append("restart")
    pipe.scheduler.operator = Op()
    pipe(prompt_embeds=pe, audio_length_in_s=0.4, num_inference_steps=3, show_progress=False, measurement=torch.zeros(2, 6400),
         output_type="latent")
    assert pipe.nan_restarts == 1 and log == ["reset", "restart"]


def test_new_entry_points_are_additive():
    """ABI version 4 stays; the new symbols are declared, bound, weak in the op library and checked by name at load; each op has its
    ctypes twin."""
    from diffmusic_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "diffmusic_hip.h")).read()
    src = open(os.path.join(ROOT, "diffmusic_amd", "csrc_torch", "torch_ops.cpp")).read()
    assert "#define DMX_ABI_VERSION 4 " in hdr and _lib.ABI_VERSION == 4
    for s in ("dmx_fir_clip_fwd", "dmx_fir_clip_bwd", "dmx_fir_wgrad", "dmx_fir_wgrad_workspace_floats", "dmx_ir_update"):
        assert s in _lib._SIGS and s in _lib.ADDED_IN_V4 and f" {s}(" in hdr and f"#pragma weak {s}" in src, s
    for name in ("fir_clip_fwd", "fir_clip_bwd", "fir_wgrad", "ir_update"):
        assert name in ops.OP_NAMES and f'm.def("{name}(' in src, name
    lib = _lib.lib()
    assert lib.dmx_fir_wgrad_workspace_floats(8, 160001, 5000) == 8 * 40 * 5000            # ceil(160001 / 4096) = 40 segments
    assert lib.dmx_fir_wgrad_workspace_floats(1, 4096, 7) == 7 and lib.dmx_fir_wgrad_workspace_floats(0, 4096, 7) == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ctypes_hip.fir_clip_fwd(torch.zeros(1, 8), torch.zeros(1, 3), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ctypes_hip.fir_wgrad(torch.zeros(1, 8), torch.zeros(1, 8), 8, 3)
    h = ops.load()
    with pytest.raises(RuntimeError, match="GPU tensor"):
        h.fir_clip_fwd(torch.zeros(1, 8), torch.zeros(1, 3), 8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        h.fir_wgrad(torch.zeros(1, 8), torch.zeros(1, 8), 8, 3)
