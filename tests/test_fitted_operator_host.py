"""CPU: what the four blind operators share through `_FittedOperator` (inverse_problem/blind.py) -- the Adam arguments, the state
life-cycle before any state exists -- and the `positional_state` declaration the pipeline reads instead of naming classes."""
from types import SimpleNamespace

import pytest
import torch

from diffmusic_amd import inverse_problem as P
from diffmusic_amd.inverse_problem.blind import _FittedOperator
from diffmusic_amd.pipelines.pipeline_musicldm import MusicLDMPipeline

BLIND = (P.BlindDereverberationOperator, P.BlindEqualizationOperator, P.BlindTimeWarpOperator, P.BlindDynamicRangeOperator)
KEYWORDS = {P.BlindDereverberationOperator: ("ir", "update_ir"), P.BlindEqualizationOperator: ("curve", "update_eq"),
            P.BlindTimeWarpOperator: ("delay", "update_warp"), P.BlindDynamicRangeOperator: ("params", "update_drc")}
L = 6400


def _check(op, **kw):
    pipe = SimpleNamespace(lanes=1, scheduler=SimpleNamespace(operator=op))
    return MusicLDMPipeline._check_positional_state(pipe, **dict(dict(shard=False, group=None, lanes=None), **kw))


@pytest.mark.parametrize("cls", BLIND)
def test_adam_arguments_are_refused_by_name(cls):
    for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9,), (0.9, 0.999, 0.5), (0.9, float("nan")), ("0.9", 0.999)):
        with pytest.raises(ValueError, match=r"^betas = .*: two numbers in \[0, 1\)$"):
            cls(betas=betas)
    for eps in (-1e-8, float("nan"), float("inf"), "1e-8"):
        with pytest.raises(ValueError, match="^adam_eps = .*: a non-negative number$"):
            cls(adam_eps=eps)
    op = cls(betas=(0, 0.5), adam_eps=0)
    assert op.betas == (0.0, 0.5) and op.adam_eps == 0.0 and all(type(v) is float for v in op.betas + (op.adam_eps,))


@pytest.mark.parametrize("cls", BLIND)
def test_fresh_instance_and_hooks_without_state(cls):
    op = cls()
    assert isinstance(op, _FittedOperator) and op.k == 0 and op._m is None and op._v is None
    assert (op.pin_kwarg, op.update_kwarg) == KEYWORDS[cls]
    assert op.reset_cache() is None and op.restart() is None                               # nothing to put back: no state, no error
    op.k = 3
    op.restart()
    assert op.k == 0 and op._m is None
    op.k = 3
    op.reset_cache()
    assert op.k == 0 and op._m is None
    assert op.after_cotangent(None, 0, None, **{op.update_kwarg: False}) is None and op.k == 0      # frozen: not a step


@pytest.mark.parametrize("cls", BLIND)
def test_blind_operators_declare_positional_state(cls):
    op = cls()
    who, what = op.positional_state
    assert who == cls.__name__ and what.endswith("estimates")
    for wrapped in (op, SimpleNamespace(inner=op), SimpleNamespace(inner=SimpleNamespace(inner=op))):
        with pytest.raises(ValueError, match=rf"^{who} cannot run as clip lanes \(lanes > 1\): its {what} are indexed by batch position"):
            _check(wrapped, lanes=2)
        for kw in (dict(shard=True), dict(group=object())):
            with pytest.raises(ValueError, match=rf"^{who} cannot be sharded over ranks \(shard / group\): its {what} are indexed by batch"):
                _check(wrapped, **kw)
        assert _check(wrapped) is None and _check(wrapped, lanes=1) is None


def test_operators_without_positional_state():
    shared = (P.TimeFrequencyMaskOperator(16000, torch.ones(513, P.tf_frames(L))), P.TimeWarpOperator(16000, torch.zeros(P.warp_knots(L))))
    for op in (P.BaseOperator(), P.IdentityOperator.__new__(P.IdentityOperator)) + shared:   # (the identity's constructor makes GPU tables)
        assert op.positional_state is None
        assert _check(op, lanes=2) is None and _check(op, shard=True) is None
    per_clip = (P.TimeFrequencyMaskOperator(16000, torch.ones(2, 513, P.tf_frames(L))), P.TimeWarpOperator(16000, torch.zeros(2, P.warp_knots(L))))
    for op, state in zip(per_clip, (("TimeFrequencyMaskOperator with per-clip gains", "gains"),
                                    ("TimeWarpOperator with per-clip delay curves", "curves"))):
        assert op.positional_state == state
        with pytest.raises(ValueError, match=r"per-clip .* cannot run as clip lanes \(lanes > 1\)"):
            _check(op, lanes=2)
        with pytest.raises(ValueError, match=r"per-clip .* cannot be sharded over ranks \(shard / group\)"):
            _check(op, shard=True)


def test_stand_in_operator_without_the_attribute_passes():
    class Op:
        noiser = None
    for op in (Op(), SimpleNamespace(inner=Op()), None):
        assert not hasattr(op, "positional_state")
        assert _check(op, lanes=2) is None and _check(op, shard=True) is None
