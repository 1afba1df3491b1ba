"""CPU: the dead span of an inpainting mask (`BaseOperator.dead_span`) and the row arithmetic of the vocoder's dead-row plan
(`dmx_conv_dead_rows`, the per-layer step csrc/hifigan.hip walks the layer list with) against a brute-force dependency walk."""
import ctypes as C

import numpy as np
import pytest
import torch


def _inpainting(mask_type, n=16000, **kw):
    """A MusicInpaintingOperator without its GPU front end: the mask is all `dead_span` looks at."""
    from diffmusic_amd.inverse_problem.operator import MusicInpaintingOperator
    op = object.__new__(MusicInpaintingOperator)
    op.audio_length_in_s, op.sample_rate, op.mask_type = n / 16000, 16000, mask_type
    op.start_inpainting_s, op.end_inpainting_s = kw.get("start"), kw.get("end")
    op.mask_percentage, op.interval_s, op.mask_duration_s = kw.get("pct", 0.3), kw.get("interval", 0.2), kw.get("dur", 0.1)
    op.mask = op.generate_mask()
    return op


def _brute_run(mask):
    best, i, m = None, 0, np.asarray(mask).reshape(-1)
    while i < len(m):
        if m[i] == 0:
            j = i
            while j < len(m) and m[j] == 0:
                j += 1
            if best is None or j - i > best[1] - best[0]:
                best = (i, j)
            i = j
        else:
            i += 1
    return best


@pytest.mark.parametrize("start,end,want", [(0.25, 0.5, (4000, 8000)), (0.0, 0.3, (0, 4800)), (0.6, 1.0, (9600, 16000)), (0.5, 0.5, None)])
def test_box_masks(start, end, want):
    op = _inpainting("box", start=start, end=end)
    assert op.dead_span(16000) == want
    assert op.dead_span(16000) == want                     # the cached answer
    assert op.dead_span(15999) is None                     # not this mask's length: no claim


def test_random_and_periodic_masks_report_their_longest_zero_run():
    torch.manual_seed(5)
    for op in (_inpainting("random", pct=0.4, dur=0.05), _inpainting("periodic", interval=0.2, dur=0.1), _inpainting("periodic", interval=0.3, dur=0.07)):
        span = op.dead_span(16000)
        assert span == _brute_run(op.mask.numpy()) and span is not None
        s0, s1 = span
        assert float(op.mask[0, s0:s1].abs().max()) == 0.0
        assert (s0 == 0 or op.mask[0, s0 - 1] != 0) and (s1 == 16000 or op.mask[0, s1] != 0)


def test_a_changed_mask_is_looked_at_again():
    op = _inpainting("box", start=0.25, end=0.5)
    assert op.dead_span(16000) == (4000, 8000)
    op.mask[0, 4100] = 1.0                                  # in place: the version counter moves
    assert op.dead_span(16000) == (4101, 8000)
    op.mask = torch.ones(1, 16000)
    assert op.dead_span(16000) is None


def test_every_other_operator_reports_none():
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.inverse_problem.operator import BaseOperator
    from diffmusic_amd.inverse_problem.track import TrackOperator
    for cls in (P.IdentityOperator, P.DeclippingOperator, P.SuperResolutionOperator, P.PhaseRetrievalOperator,
                P.MusicDereverberationOperator, P.StyleGuidanceOperator):
        assert cls.dead_span is BaseOperator.dead_span, cls
        assert object.__new__(cls).dead_span(16000) is None, cls
    track = object.__new__(TrackOperator)
    track.inner = _inpainting("box", start=0.25, end=0.5)   # even around an inpainting operator: the windows overlap
    assert track.dead_span(16000) is None


# ---- the plan's row arithmetic ---------------------------------------------------------------------------------------------------------
def _lib():
    from diffmusic_amd import _lib as L
    from diffmusic_amd.build import build_library
    build_library()
    h = C.CDLL(L.LIB_PATH)
    h.dmx_conv_dead_rows.restype = C.c_int
    h.dmx_conv_dead_rows.argtypes = [C.c_int] * 9 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return h


def _dead_rows(h, layer, t_in, t_out, span):
    k, dil, pad, stride, tr = layer
    lo, hi = C.c_int(), C.c_int()
    assert h.dmx_conv_dead_rows(k, dil, pad, stride, tr, t_in, t_out, span[0], span[1], C.byref(lo), C.byref(hi)) == 0
    return lo.value, hi.value


def _out_len(layer, t):
    k, dil, pad, stride, tr = layer
    return (t - 1) * stride - 2 * pad + k if tr else t + 2 * pad - dil * (k - 1)


def _deps(layer, t_in):
    """D[t, u]: output row t of the layer reads input row u."""
    k, dil, pad, stride, tr = layer
    t_out = _out_len(layer, t_in)
    D = np.zeros((t_out, t_in), dtype=bool)
    for u in range(t_in):
        for j in range(k):
            t = u * stride - pad + j if tr else u + pad - j * dil
            if 0 <= t < t_out:
                D[t, u] = True
    return D


def _as_set(span):
    return set(range(span[0], span[1]))


# (k, dilation, padding, stride, transposed): a small vocoder -- upsampler, two resblock steps (dilated conv, conv, residual), upsampler,
# one more step, the output convolution
UP1, UP2, POST = (4, 1, 1, 2, 1), (8, 1, 2, 4, 1), (7, 1, 3, 1, 0)
STEPS1 = [((3, 1, 1, 1, 0), (3, 1, 1, 1, 0)), ((5, 3, 6, 1, 0), (5, 1, 2, 1, 0))]
STEPS2 = [((11, 5, 25, 1, 0), (11, 1, 5, 1, 0))]


@pytest.mark.parametrize("t0,hole", [(37, (90, 250)), (37, (0, 170)), (37, (120, 296)), (37, (100, 130)), (23, (1, 183)), (23, (50, 60))])
def test_plan_rows_against_a_brute_force_dependency_walk(t0, hole):
    """Every tensor of the chain: the rows the interval arithmetic calls dead are exactly the rows from which no path of the dependency
    graph reaches a sample outside the hole."""
    h = _lib()
    t1 = _out_len(UP1, t0)
    t2 = _out_len(UP2, t1)
    assert _out_len(POST, t2) == t2 == 8 * t0 and hole[1] <= t2
    live = np.ones(t2, dtype=bool)
    live[hole[0]:hole[1]] = False

    def reach_back(reach_out, layer, t_in):                # rows of the input from which a live sample is reached through this layer
        return (_deps(layer, t_in)[reach_out].any(axis=0)) if reach_out.any() else np.zeros(t_in, dtype=bool)

    # backwards, brute force and interval arithmetic side by side
    reach, span = reach_back(live, POST, t2), _dead_rows(h, POST, t2, t2, hole)
    checked = 0

    def check(name):
        nonlocal checked
        assert set(np.flatnonzero(~reach)) == _as_set(span), (name, span, np.flatnonzero(~reach)[[0, -1]] if (~reach).any() else None)
        checked += 1

    check("stage 2 output")
    for steps, up, t_len, t_prev in ((STEPS2, UP2, t2, t1), (STEPS1, UP1, t1, t0)):
        for c1, c2 in reversed(steps):
            r_h, s_h = reach_back(reach, c2, t_len), _dead_rows(h, c2, t_len, t_len, span)
            assert set(np.flatnonzero(~r_h)) == _as_set(s_h)
            s_x = _dead_rows(h, c1, t_len, t_len, s_h)
            reach = reach_back(r_h, c1, t_len) | reach      # the residual: the row itself
            span = (max(s_x[0], span[0]), min(s_x[1], span[1]))
            span = span if span[1] > span[0] else (0, 0)
            check("step input")
        reach, span = reach_back(reach, up, t_prev), _dead_rows(h, up, t_prev, t_len, span)
        check("upsampler input")
    assert checked == 6
    if hole[1] - hole[0] < 40:
        assert span == (0, 0)                               # a short hole dies out on the way down


def test_dead_rows_edges():
    h = _lib()
    conv = (7, 1, 3, 1, 0)
    assert _dead_rows(h, conv, 100, 100, (20, 60)) == (23, 57)
    assert _dead_rows(h, conv, 100, 100, (0, 60)) == (0, 57)            # a hole at the clip's start extends past it
    assert _dead_rows(h, conv, 100, 100, (20, 100)) == (23, 100)
    assert _dead_rows(h, conv, 100, 100, (20, 26)) == (0, 0)            # shorter than the kernel: nothing
    assert _dead_rows(h, conv, 100, 100, (60, 20)) == (0, 0)
    assert _dead_rows(h, conv, 100, 100, (-5, 400)) == (0, 100)
    up = (4, 1, 1, 2, 1)                                                  # in[u] -> out[2u - 1 .. 2u + 2]
    assert _dead_rows(h, up, 50, 100, (20, 60)) == (11, 29)
    assert _dead_rows(h, up, 50, 100, (0, 60)) == (0, 29)
    assert _dead_rows(h, up, 50, 100, (21, 100)) == (11, 50)
