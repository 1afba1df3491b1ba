"""CPU: the host side of the measurement noise inside the guided step (diffmusic_amd/inverse_problem/noise.py): the noiser registry and
its streams, which noisers take part in a step, the pipeline's refusal of the process-wide stream under clip lanes / clip sharding,
and the new C-ABI symbols / ops in both bindings.  No HIP launch anywhere."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dmx_audio_guidance_fwd_ex", "dmx_audio_guidance_bwd_ex", "dmx_noise_add")
NEW_OPS = ("mel_guidance", "noise_add")


def test_get_noiser_streams():
    from diffmusic_amd import inverse_problem as P
    n = P.get_noiser("gaussian", 0.05, stream="clip")
    assert isinstance(n, P.GaussianNoise) and n.sigma == 0.05 and n.stream == "clip" and n.additive_sigma == 0.05
    assert P.get_noiser("gaussian", 0.05).stream == "global"                  # the reference's semantics stay the default
    assert P.get_noiser(name="gaussian", sigma=0.0).additive_sigma == 0.0     # the call `get_noiser(**cfg.inverse_problem.noise)` makes
    with pytest.raises(ValueError, match="stream"):
        P.get_noiser("gaussian", 0.05, stream="per_call")
    with pytest.raises(ValueError, match="Unknown noise"):
        P.get_noiser("laplace", 0.05)


def test_only_an_explicit_additive_sigma_makes_a_noisy_step():
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.inverse_problem.noise import step_sigma
    assert step_sigma(P.GaussianNoise(0.05)) == 0.05
    assert step_sigma(P.GaussianNoise(0.0)) == 0.0 and step_sigma(None) == 0.0
    poisson = P.get_noiser("poisson", 1.0)
    assert isinstance(poisson, P.PoissonNoise) and step_sigma(poisson) == 0.0
    poisson.sigma = 0.3                                                       # an attribute called sigma is not what decides
    assert step_sigma(poisson) == 0.0
    assert step_sigma(SimpleNamespace(sigma=0.3)) == 0.0


def test_sigma_zero_forward_is_the_identity_and_leaves_the_global_rng_alone():
    from diffmusic_amd import inverse_problem as P
    torch.manual_seed(5)
    before = torch.get_rng_state()
    x = torch.arange(6.0).reshape(2, 3)
    assert P.GaussianNoise(0.0)(x) is x
    assert torch.equal(torch.get_rng_state(), before)


def test_clip_key_is_a_function_of_seed_and_step_only():
    from diffmusic_amd.inverse_problem.noise import MEASUREMENT_KEY_XOR, clip_noise_key
    key, off = clip_noise_key(7, 3)
    assert key & 0xFFFFFFFFFFFFFFFF == 7 ^ MEASUREMENT_KEY_XOR and off == 3 << 32
    assert -(1 << 63) <= key < (1 << 63)                                      # fits the op schema's signed int
    assert clip_noise_key(7, 3) != clip_noise_key(7, 4) and clip_noise_key(7, 3)[0] != clip_noise_key(8, 3)[0]
    big, _ = clip_noise_key((1 << 63) + 5, 0)                                 # seeds with the top bit set stay in range
    assert -(1 << 63) <= big < (1 << 63) and big & 0xFFFFFFFFFFFFFFFF == ((1 << 63) + 5) ^ MEASUREMENT_KEY_XOR
    assert key != 7                                                           # never the sampler's key for the same generator


def test_clip_stream_refuses_a_draw_without_its_key():
    from diffmusic_amd import inverse_problem as P
    n = P.GaussianNoise(0.05, stream="clip")
    with pytest.raises(ValueError, match="step index"):
        n.draw((2, 8), "cpu", step=None, generator=[torch.Generator(), torch.Generator()])
    with pytest.raises(ValueError, match="step index"):
        n.draw((2, 8), "cpu", step=0, generator=None)
    with pytest.raises(ValueError, match="one generator per clip"):
        n.draw((2, 8), "cpu", step=0, generator=[torch.Generator()])


def test_scheduler_hands_step_index_and_generators_to_a_noisy_operator_only():
    from diffmusic_amd import inverse_problem as P
    from tests.stubs import SCHED, CpuScheduler
    gens = [torch.Generator().manual_seed(3)]
    s = CpuScheduler(operator=SimpleNamespace(noiser=P.GaussianNoise(0.05, stream="clip")), **SCHED)
    s.set_timesteps(4)
    t2 = s._timesteps_host[2]
    assert s._op_kwargs(None, t2, gens) == dict(step=2, generator=gens)
    assert s._op_kwargs(dict(ir=1), t2, gens) == dict(ir=1, step=2, generator=gens)
    forced = dict(noise=torch.zeros(1, 4))
    assert s._op_kwargs(forced, t2, gens) is forced                            # teacher forcing: no draw, nothing added
    for quiet in (None, SimpleNamespace(noiser=None), SimpleNamespace(noiser=P.GaussianNoise(0.0)), SimpleNamespace(noiser=P.PoissonNoise(1.0))):
        s.operator = quiet
        assert s._op_kwargs(None, t2, gens) is None                            # sigma = 0: the call guidance() gets is today's


def _call(pipe, B, **kw):
    pe = torch.nn.functional.normalize(torch.randn(B, 512, generator=torch.Generator().manual_seed(1)), dim=-1)
    return pipe(prompt_embeds=pe, audio_length_in_s=0.4, num_inference_steps=3, measurement=torch.zeros(B, 6400), show_progress=False,
                output_type="latent", generator=[torch.Generator().manual_seed(k) for k in range(B)], **kw)


@pytest.mark.parametrize("how", [dict(lanes=2), dict(shard=True)])
def test_pipeline_refuses_the_global_noise_stream_under_lanes_and_sharding(how):
    """The check reads `scheduler.operator.noiser` and needs nothing else of the operator (here: a plain object, no HIP handle)."""
    from diffmusic_amd import inverse_problem as P
    from tests.stubs import make_pipeline
    pipe = make_pipeline()
    pipe.scheduler.operator = SimpleNamespace(noiser=P.GaussianNoise(0.05))
    with pytest.raises(ValueError, match="per-clip noise stream"):
        _call(pipe, 4, **how)
    assert pipe.scheduler.calls == 0


@pytest.mark.parametrize("noiser", ["clip", "zero", "poisson", "none"])
def test_pipeline_lets_clip_stream_and_silent_noisers_through_lanes(noiser):
    from diffmusic_amd import inverse_problem as P
    from tests.stubs import make_pipeline
    n = dict(clip=P.GaussianNoise(0.05, stream="clip"), zero=P.GaussianNoise(0.0), poisson=P.PoissonNoise(1.0), none=None)[noiser]
    pipe = make_pipeline()
    pipe.scheduler.operator = SimpleNamespace(noiser=n)
    out = _call(pipe, 4, lanes=2).audios
    assert out.shape[0] == 4 and pipe.scheduler.calls == 2 * 3
    # sharding: the noise check passes, the next one (no process group here) is the one that speaks
    with pytest.raises(RuntimeError, match="process group"):
        _call(pipe, 4, shard=True)


def test_global_stream_runs_in_the_plain_loop():
    from diffmusic_amd import inverse_problem as P
    from tests.stubs import make_pipeline
    pipe = make_pipeline()
    pipe.scheduler.operator = SimpleNamespace(noiser=P.GaussianNoise(0.05))
    assert _call(pipe, 2).audios.shape[0] == 2


def test_new_symbols_are_declared_exported_and_bound():
    from diffmusic_amd import _lib
    from diffmusic_amd.build import build_library
    hdr = open(os.path.join(ROOT, "include", "diffmusic_hip.h")).read()
    h = ctypes.CDLL(build_library())
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(h, name), name
        assert name in _lib._SIGS, name
    # additive: the version the other checks pin does not move, and the old pair keeps its argument lists
    assert _lib.ABI_VERSION == 4 and "#define DMX_ABI_VERSION 4" in hdr
    assert len(_lib._SIGS["dmx_audio_guidance_fwd_ex"][1]) == len(_lib._SIGS["dmx_audio_guidance_fwd"][1]) + 4
    assert len(_lib._SIGS["dmx_audio_guidance_bwd_ex"][1]) == len(_lib._SIGS["dmx_audio_guidance_bwd"][1]) + 4


def test_new_ops_exist_in_both_bindings():
    from diffmusic_amd import ops
    from diffmusic_amd.build import build_torch_ops
    assert os.path.exists(build_torch_ops())
    h = ops.load()
    for name in NEW_OPS:
        assert name in ops.OP_NAMES and callable(getattr(ops.ctypes_hip, name))
        assert str(getattr(h, name).default._schema).startswith(f"diffmusic_hip::{name}(")
    args = [a.name for a in h.mel_guidance.default._schema.arguments]
    assert args[-4:] == ["noise", "noise_mag", "sigma", "thr"] and args[-5] == "gscale"   # the one op carries the noise and the clip
    with pytest.raises(RuntimeError, match="GPU tensor"):
        h.noise_add(torch.zeros(4), torch.zeros(4), 0.5)                                   # no CPU fallback
