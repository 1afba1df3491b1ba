"""CPU: the mathematics, the bound and the host side of the blind de-compression (csrc/drc_fit.hip, BlindDynamicRangeOperator; DESIGN.md
section 8.12).  The five parameter gradients against float64 central differences of `drc_cases.model` and against torch autograd through a
restatement of the recurrence; both forms of gm; the fp32 emulation inside the bound and every mutant outside it; the update's boxes, its
frozen parameters and the table it derives; the float64 recovery loop under half of the GPU test's bounds; the operator's and the example's
refusals.  tests/test_gpu_blind_drc.py holds the kernels to the same bound."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import drc_cases as D
from tests import drc_fit_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
GRAD_CASES = ["L6400", "L6400_hard"]


def _loss64(c, b, phi):
    """<dy, A_phi x> of clip b through drc_cases.model at the parameters phi = (T, k, m, ln aA, ln aR)"""
    i = F.inputs(c)
    P = D.SimpleNamespace(T=phi[0], k=phi[1], W=c.W, aA=math.exp(phi[3]), aR=math.exp(phi[4]), makeup=phi[2],
                          kq=phi[1] / (2.0 * c.W) if c.W > 0 else 0.0)
    return float((D.model(i.x[b:b + 1], c.L, P).y[0] * i.dy[b].astype(f64)).sum())


def _grad64(c):
    """the model's five gradients (B, 5) with the model's own tape"""
    return F.model_part(c).sum(1)


# ---- the mathematics --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradients_against_central_differences_of_the_model(name):
    c = F.CASE[name]
    g = _grad64(c)
    h = 1e-6
    for b in range(c.B):
        phi = F.phi_of(c.P[b])
        for q in range(F.NP):
            up, dn = phi.copy(), phi.copy()
            up[q] += h
            dn[q] -= h
            fd = (_loss64(c, b, up) - _loss64(c, b, dn)) / (2 * h)
            rel = abs(fd - g[b, q]) / abs(g[b, q])
            print(f"{name} clip {b} {F.NAMES[q]}: model {g[b, q]:+.9e}  central difference {fd:+.9e}  rel {rel:.1e}")
            assert rel <= 1e-6, (name, b, F.NAMES[q], g[b, q], fd)


def _torch_forward(x, L, phi, W):
    """the definition of DESIGN.md 8.9 in torch float64, differentiable in phi (5,); x (L,)"""
    H = D.blocks(L)
    xb = torch.zeros(H * D.R, dtype=torch.float64)
    xb[:L] = x
    p = (xb.reshape(H, D.R) ** 2).mean(1)
    T, k, mk, aA, aR = phi[0], phi[1], phi[2], torch.exp(phi[3]), torch.exp(phi[4])
    d = 10.0 * torch.log10(p + D.EPS) - T
    t = d + 0.5 * W
    knee = k * t * t / (2.0 * W) if W > 0 else torch.zeros_like(d)
    cc = torch.where(2.0 * d < -W, torch.zeros_like(d), torch.where(2.0 * d <= W, knee, k * d))
    s, rows = torch.zeros((), dtype=torch.float64), []
    for j in range(H):
        s = s + torch.where(cc[j] > s, aA, aR) * (cc[j] - s)
        rows.append(s)
    G = 10.0 ** ((mk - torch.stack(rows)) / 20.0)
    Gp = torch.cat([(10.0 ** (mk / 20.0)).reshape(1), G[:-1]])
    w = (torch.arange(D.R, dtype=torch.float64) + 1.0) / D.R
    g = (Gp[:, None] + w[None] * (G - Gp)[:, None]).reshape(-1)[:L]
    return g * x


@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradients_against_torch_autograd_through_the_recurrence(name):
    c = F.CASE[name]
    i = F.inputs(c)
    g = _grad64(c)
    for b in range(c.B):
        phi = torch.tensor(F.phi_of(c.P[b]), dtype=torch.float64, requires_grad=True)
        y = _torch_forward(torch.from_numpy(i.x[b].astype(f64)), c.L, phi, c.W)
        assert float((y.detach() - torch.from_numpy(F.forward(c)[b][0].y[0])).abs().max()) <= 1e-12
        (ag,) = torch.autograd.grad((y * torch.from_numpy(i.dy[b].astype(f64))).sum(), phi)
        rel = np.abs(ag.numpy() - g[b]) / np.abs(g[b])
        print(f"{name} clip {b}: autograd vs model, relative {rel}")
        assert bool((rel <= 1e-9).all()), (name, b, rel)


@pytest.mark.parametrize("c", F.CASES, ids=lambda c: c.name)
def test_both_forms_of_the_makeup_gradient_agree(c):
    i = F.inputs(c)
    g = _grad64(c)
    for b in range(c.B):
        y = F.forward(c)[b][0].y[0]
        other = D.LN10_20 * float((i.dy[b].astype(f64) * y).sum())
        scale = D.LN10_20 * float(np.abs(i.dy[b].astype(f64) * y).sum())
        assert abs(other - g[b, 2]) <= 1e-8 * max(scale, 1e-300), (c.name, b, other, g[b, 2])


def test_the_vectorised_restatement_is_the_model():
    """fwd64 / pgrad64, which the recovery loop runs with one parameter row per clip, against drc_cases.model and model_pgrad"""
    for name in ("L6400", "L6400_hard", "L1000"):
        c = F.CASE[name]
        i = F.inputs(c)
        phi = np.stack([F.phi_of(P) for P in c.P])
        r = F.fwd64(i.x.astype(f64), c.L, phi, c.W)
        for b in range(c.B):
            assert float(np.abs(r.y[b] - F.forward(c)[b][0].y[0]).max()) <= 1e-13
        g, want = F.pgrad64(i.x.astype(f64), i.dy.astype(f64), c.L, r), _grad64(c)
        assert float(np.abs(g - want).max()) <= 1e-12 * float(np.abs(want).max())


def test_a_clip_below_the_knee_has_exactly_zero_gradients_except_makeup():
    c = F.CASE["L6400_quiet_clip"]
    part = F.model_part(c)
    assert not part[2][:, [0, 1, 3, 4]].any() and part[2][:, 2].any() and part[0][:, [0, 1, 3, 4]].any()
    em = F.emulate_case(c)
    assert not em[2].part[:, [0, 1, 3, 4]].any() and not em[2].e.tape.any()


# ---- the bound --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", F.CASES, ids=lambda c: c.name)
def test_emulation_lies_within_the_bound_in_every_element(c):
    em = F.emulate_case(c)
    tapes = [e.e.tape[0] for e in em]
    for b in range(c.B):
        r, q = F.forward(c)[b]
        assert D.tape_differences_allowed(em[b].e.tape, r, q), (c.name, b)
    part = np.stack([e.part for e in em])
    rp = F.judge_pgrad(c, part, tapes)
    u = F.update_setup(c)
    got = F.emulate_update(part, u, c.W)
    ru = F.judge_update(c, part, got)
    print(f"{c.name}: largest |emulation - model| / bound: part {rp:.4f}  update {ru:.4f}")
    assert rp <= 1.0 and ru <= 1.0, (c.name, rp, ru)


@pytest.mark.parametrize("c", F.CASES, ids=lambda c: c.name)
def test_no_block_of_a_case_is_ambiguous_beyond_the_cap(c):
    """the condition of the GPU test's tape rule, from the float64 model alone: none for H < 100, at most AMBIG_CAP of the blocks else"""
    for b in range(c.B):
        share = D.ambiguous_share(F.forward(c)[b][1])
        assert share <= (D.AMBIG_CAP if c.H >= 100 else 0.0), (c.name, b, share)


@pytest.mark.parametrize("mut", sorted(F.MUTANTS))
def test_every_mutant_leaves_the_bound(mut):
    stage, names = F.MUTANTS[mut]
    ratios = [F.run_mutant(F.CASE[n], mut, stage) for n in names]
    print(f"{mut} ({stage}): {dict(zip(names, ratios))}")
    assert max(ratios) > 1.0, (mut, ratios)
    assert len(F.MUTANTS) >= 8


def test_cases_cover_what_the_kernels_can_get_wrong():
    by = {c.name: c for c in F.CASES}
    assert {1, 63, 65, 1000, 6400, 20037, 70000} <= {c.L for c in F.CASES}
    assert all(c.B == 3 and len({tuple(F.phi_of(P)) for P in c.P}) == 3 for c in F.CASES), "a different row per clip"
    assert by["L70000"].nseg == 5 and by["L70000"].H % F.SEG != 0 and by["L20037_stride"].stride > by["L20037_stride"].full > 20037
    assert by["L20037_stride"].off % 4 != 0 and by["L6400_hard"].W == 0.0 and by["L6400_limiter"].P[0].k == 1.0
    assert by["L6400_fastrel"].P[0].aA < by["L6400_fastrel"].P[0].aR
    assert all(c.why for c in F.CASES)


# ---- the update -------------------------------------------------------------------------------------------------------------------------
def _contract_ok(theta, W):
    T, k, mk, aA, aR, bA, bR, kq = theta.T
    ok = (np.abs(T) <= 200).all() and (np.abs(mk) <= 200).all() and ((k >= 0) & (k <= 1)).all() and ((aA > 0) & (aA <= 1)).all() and \
        ((aR > 0) & (aR <= 1)).all()
    derived = np.array_equal(bA, (1.0 - aA.astype(f64)).astype(f32)) and np.array_equal(bR, (1.0 - aR.astype(f64)).astype(f32)) and \
        np.array_equal(kq, (k.astype(f64) / (2.0 * W)).astype(f32) if W > 0 else np.zeros_like(k))
    return bool(ok and derived)


def test_update_chains_stay_inside_the_boxes_and_the_contract_of_drc_fwd():
    """200 updates from hostile gradients (huge, alternating, one-sided): phi stays inside the box, every table row inside what dmx_drc_fwd
    accepts, the derived entries are the double-rounded-once ones"""
    c = F.CASE["L6400"]
    u = F.update_setup(c)
    u.lo, u.hi = F.REC_BOX
    u.lr = F.LR
    rng = np.random.default_rng(5)
    push = np.array([[1e6, -1e6, 1e6, -1e6, 1e6], [-1e6, 1e6, -1e6, 1e6, -1e6], [1.0, 1.0, 1.0, 1.0, 1.0]])
    for k in range(1, 201):
        u.k = k
        part = (push * rng.standard_normal((3, 1)) if k % 3 else push)[:, None, :].astype(f32)
        u.phi, u.m, u.v, u.theta = F.emulate_update(part, u, c.W)
        assert bool((u.phi >= np.array(u.lo, f32)).all() and (u.phi <= np.array(u.hi, f32)).all()), k
        assert _contract_ok(u.theta, c.W), k
    assert bool((u.phi == np.array(u.lo, f32)).any() or (u.phi == np.array(u.hi, f32)).any()), "the box acted"


def test_a_frozen_parameter_keeps_value_moments_and_table_entries():
    c = F.CASE["L65"]
    u = F.update_setup(c)
    assert u.lr[4] == 0.0 and all(a > 0 for a in u.lr[:4])
    part = F.model_part(c).astype(f32)
    phi, m, v, theta = F.emulate_update(part, u, c.W)
    assert np.array_equal(phi[:, 4], u.phi[:, 4]) and np.array_equal(m[:, 4], u.m[:, 4]) and np.array_equal(v[:, 4], u.v[:, 4])
    assert np.array_equal(theta[:, [4, 6]], u.theta[:, [4, 6]])
    assert not np.array_equal(phi[:, :4], u.phi[:, :4]) and not np.array_equal(m[:, :4], u.m[:, :4])
    mphi, mm, mv, mtheta, _ = F.model_update(part, u, c.W)
    assert np.array_equal(mphi[:, 4], u.phi[:, 4].astype(f64)) and np.array_equal(mtheta[:, [4, 6]], u.theta[:, [4, 6]].astype(f64))


def test_the_box_of_the_update_setup_acts():
    for c in F.CASES:
        u = F.update_setup(c)
        phi = F.model_update(F.model_part(c), u, c.W)[0]
        assert bool((u.phi[:, 0] < f32(u.lo[0])).any()), c.name            # a clip starts under the threshold floor
        assert bool((phi[:, 0] == float(f32(u.lo[0]))).any()), c.name


def test_drc_table_derives_what_the_launcher_derives():
    from diffmusic_amd.inverse_problem import dsp
    src = open(os.path.join(ROOT, "diffmusic_amd", "csrc", "drc.hip")).read()
    assert "(float)((double)slope / (2.0 * (double)knee))" in src and "(float)(1.0 - (double)aA)" in src      # what is restated here
    for c in F.CASES:
        t = F.table(c)
        assert t.dtype == f32 and t.shape == (3, 8) and _contract_ok(t, c.W)
        for b, P in enumerate(c.P):
            assert tuple(t[b, :5].astype(f64)) == (P.T, P.k, P.makeup, P.aA, P.aR)
            assert float(t[b, 7]) == float(f32(P.kq))
    one = dsp.drc_table(-24.0, 0.75, 0.5, 0.25, 3.0, 6.0, 4)
    assert one.shape == (4, 8) and (one == one[0]).all() and tuple(one[0]) == (-24.0, 0.75, 3.0, 0.5, 0.25, 0.5, 0.75, f32(0.0625))
    for bad in (dict(batch=0), dict(knee_db=-1.0), dict(knee_db=float("nan")), dict(threshold_db=[1.0, 2.0])):
        kw = dict(threshold_db=-24.0, slope=0.75, a_att=0.5, a_rel=0.25, makeup_db=0.0, knee_db=6.0, batch=3)
        kw.update(bad)
        with pytest.raises(ValueError):
            dsp.drc_table(**kw)
    assert np.allclose(dsp.drc_time_ms(dsp.drc_coeffs(16000, 5.0, 100.0), 16000), [5.0, 100.0], rtol=1e-6)


# ---- recovery ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(F.REC_FITS))
def test_the_float64_recovery_loop_stays_under_half_of_every_bound(which):
    o = F.recovery_loop_float64(F.REC_FITS[which])
    err = o.err.max(0)
    print(f"recovery in float64, fit = {which}, seeds {F.REC_SEEDS}: residual {o.first} -> {o.last}; worst |dT| {err[0]:.3f} dB  |dk| {err[1]:.4f}  "
          f"|dm| {err[2]:.4f} dB  |d ln a| {max(err[3], err[4]):.4f}")
    Bd = F.REC_BOUNDS
    assert bool((o.first > Bd["start_residual"]).all())
    assert float(o.last.max()) < 0.5 * Bd["residual"] and err[0] < 0.5 * Bd["T"] and err[1] < 0.5 * Bd["k"] and err[2] < 0.5 * Bd["m"]
    assert max(err[3], err[4]) < 0.5 * Bd["ln_a"]
    if which == "three":
        assert not o.err[:, 3:].any(), "the times stay at the truth"


# ---- the operator and the plumbing --------------------------------------------------------------------------------------------------------
def test_operator_construction_refusals_by_name():
    from diffmusic_amd import inverse_problem as P
    op = P.BlindDynamicRangeOperator()
    assert op.fit == ("threshold", "ratio", "makeup") and op.lr == (0.25, 0.01, 0.1, 0.0, 0.0) and op.knee_db == 6.0 and op.k == 0
    assert op.drc_estimate is None and op.phi_estimate is None and op.true_params is None
    assert op.box_lo[:3] == (-60.0, 0.0, -24.0) and op.box_hi[:3] == (0.0, 1.0, 24.0)
    assert math.isclose(op.box_lo[3], F.LN_LO, rel_tol=1e-6) and math.isclose(op.box_hi[3], F.LN_HI, rel_tol=1e-4)
    assert np.allclose(op._start, F.rows_phi([dict(threshold_db=-12, ratio=2, attack_ms=5, release_ms=100, makeup_db=0)])[0])
    five = P.BlindDynamicRangeOperator(fit=("threshold", "ratio", "makeup", "attack", "release"), lr=dict(attack=0.5))
    assert five.lr == (0.25, 0.01, 0.1, 0.5, 0.02)
    for name, kw in (("sample_rate", dict(sample_rate=0)), ("knee_db", dict(knee_db=-1.0)), ("knee_db", dict(knee_db=float("inf"))),
                     ("fit", dict(fit=("threshold", "knee"))), ("fit", dict(fit=())), ("fit", dict(fit=("ratio", "ratio"))),
                     ("init", dict(init=dict(threshold=-12.0))), ("ratio", dict(init=dict(ratio=0.5))), ("attack_ms", dict(init=dict(attack_ms=0.0))),
                     ("init", dict(init=dict(threshold_db=-70.0))), ("init", dict(init=dict(attack_ms=0.1))), ("init", dict(init=dict(makeup_db=30.0))),
                     ("lr", dict(lr=dict(knee=0.1))), ("lr", dict(lr=dict(slope=0.0))), ("lr", dict(lr=dict(makeup=float("nan")))),
                     ("betas", dict(betas=(0.9, 1.0))), ("adam_eps", dict(adam_eps=-1.0)), ("threshold_range", dict(threshold_range=(0.0, -60.0))),
                     ("threshold_range", dict(threshold_range=(-300.0, 0.0))), ("makeup_range", dict(makeup_range=(-24.0,))),
                     ("time_range_ms", dict(time_range_ms=(0.0, 100.0))), ("time_range_ms", dict(time_range_ms=(100.0, 1.0)))):
        with pytest.raises(ValueError, match=name):
            P.BlindDynamicRangeOperator(**kw)
    with pytest.raises(ValueError, match="params"):
        op.forward(torch.zeros(1, 64))                                      # no true parameters given or kept; refused before any GPU work
    with pytest.raises(ValueError, match="params"):
        op.forward(torch.zeros(1, 64), params=dict(threshold_db=-24.0))
    with pytest.raises(ValueError, match="ratio"):
        op.forward(torch.zeros(1, 64), params=dict(F.REC_TRUE, ratio=0.5))
    assert "lr" in P.BlindDynamicRangeOperator.__doc__ and "not tuned" in P.BlindDynamicRangeOperator.__doc__


def test_ops_are_registered_in_both_bindings_with_full_schemas():
    from diffmusic_amd import ops, _lib
    src = open(os.path.join(ROOT, "diffmusic_amd", "csrc_torch", "torch_ops.cpp")).read()
    for name in ("drc_fwd_p", "drc_bwd_p", "drc_pgrad", "drc_update"):
        assert name in ops.OP_NAMES and f"dmx_{name}" in _lib.ADDED_IN_V4 and f"dmx_{name}" in _lib._SIGS
        assert re.search(rf'm\.def\("{name}\(Tensor ', src)
    assert "drc_fwd_p(Tensor x, int L, Tensor theta, float knee_db) -> (Tensor, Tensor, Tensor)" in src
    assert "Tensor(a!) phi, Tensor(b!) m, Tensor(c!) v, Tensor(d!) theta" in src
    assert _lib.ABI_VERSION == 4
    hdr = open(os.path.join(ROOT, "include", "diffmusic_hip.h")).read()
    assert "#define DMX_ABI_VERSION 4" in hdr and all(f"int dmx_{n}(" in hdr for n in ("drc_fwd_p", "drc_bwd_p", "drc_pgrad", "drc_update"))
    with pytest.raises((RuntimeError, AssertionError)):
        ops.ctypes_hip.drc_fwd_p(torch.zeros(1, 300), 300, torch.zeros(1, 8), 6.0)          # no CPU fallback
    com = open(os.path.join(ROOT, "diffmusic_amd", "csrc", "drc_common.h")).read()
    for k in ("drc.hip", "drc_fit.hip"):
        assert '#include "drc_common.h"' in open(os.path.join(ROOT, "diffmusic_amd", "csrc", k)).read()
    assert "level_over_threshold" in com and "curve_by_region" in com


def test_pipelines_refuse_lanes_and_shards_by_name():
    """The pipeline builds both refusals from the operator's `positional_state`, so the full texts are checked where they are raised."""
    from diffmusic_amd.pipelines.pipeline_audioldm2 import AudioLDM2Pipeline
    from diffmusic_amd.pipelines.pipeline_musicldm import MusicLDMPipeline
    assert AudioLDM2Pipeline._check_positional_state is MusicLDMPipeline._check_positional_state
    from diffmusic_amd import inverse_problem as P
    for top in (lambda op: op, lambda op: P.MixtureOperator(op, 2, [1.0, 0.5])):
        pipe = MusicLDMPipeline.__new__(MusicLDMPipeline)
        pipe.lanes = 1
        pipe.scheduler = D.SimpleNamespace(operator=top(P.BlindDynamicRangeOperator()))
        pipe._check_positional_state(False, None, None)
        with pytest.raises(ValueError) as lane:
            pipe._check_positional_state(False, None, 2)
        assert str(lane.value) == ("BlindDynamicRangeOperator cannot run as clip lanes (lanes > 1): its parameter estimates are indexed by "
                                   "batch position, and a lane sees only its own clips")
        with pytest.raises(ValueError) as rank:
            pipe._check_positional_state(True, None, None)
        assert str(rank.value) == ("BlindDynamicRangeOperator cannot be sharded over ranks (shard / group): its parameter estimates are "
                                   "indexed by batch position, and a rank sees only its own clips")


# ---- examples/run_inverse_problem.py ------------------------------------------------------------------------------------------------------
def _example():
    spec = importlib.util.spec_from_file_location("run_inverse_problem", os.path.join(ROOT, "examples", "run_inverse_problem.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_argument_rules():
    from diffmusic_amd.config import compose
    from diffmusic_amd import constants, inverse_problem as P
    mod = _example()
    assert mod.BLIND_DRC == constants.MUSIC_BLIND_DECOMPRESSION and mod.BLIND_DRC in mod.TASKS
    t = ("-t", "music_blind_decompression")

    def kw(*argv, cfg=None):
        return mod.blind_drc_params(mod.parse_args(list(argv)), cfg)
    true = dict(threshold_db=-24.0, ratio=4.0, attack_ms=5.0, release_ms=100.0, makeup_db=3.0)
    assert kw(*t) == dict(operator={}, true=true)
    got = kw(*t, "--drc_fit", "threshold,ratio,makeup,attack", "--drc_ratio", "inf", "--drc_init_ratio", "3", "--drc_knee_db", "0")
    assert got["true"] == dict(true, ratio=math.inf) and got["operator"] == dict(knee_db=0.0, fit=("threshold", "ratio", "makeup", "attack"),
                                                                                  init=dict(ratio=3.0))
    assert mod.compressor_params(mod.parse_args([*t, "--drc_ratio", "8"])) is None            # there the flags describe the measurement
    for bad in (("--drc_fit", "threshold,knee"), ("--drc_fit", ""), ("--drc_ratio", "0.5"), ("--drc_init_ratio", "0.5"), ("--drc_attack_ms", "0"),
                ("--drc_init_threshold_db", "-90"), ("--drc_knee_db", "-1"), ("--drc_init_makeup_db", "nan")):
        with pytest.raises(SystemExit):
            kw(*t, *bad)
    for other in ("music_inpainting", "music_decompression"):
        assert kw("-t", other) is None
        with pytest.raises(SystemExit, match="music_blind_decompression"):
            kw("-t", other, "--drc_fit", "threshold")
        with pytest.raises(SystemExit, match="music_blind_decompression"):
            kw("-t", other, "--drc_init_ratio", "3")
    cfg = compose("dps", overrides=["data=moises", "model=musicldm", f"inverse_problem={mod.BLIND_DRC}"])
    assert cfg.inverse_problem.noise.name == "gaussian" and float(cfg.inverse_problem.noise.sigma) == 0.0
    from_cfg = kw(*t, cfg=cfg)
    assert from_cfg["true"] == true and from_cfg["operator"]["fit"] == ("threshold", "ratio", "makeup") and from_cfg["operator"]["knee_db"] == 6.0
    assert from_cfg["operator"]["init"] == dict(threshold_db=-12.0, ratio=2.0, attack_ms=5.0, release_ms=100.0, makeup_db=0.0)
    assert from_cfg["operator"]["lr"] == dict(threshold=0.25, slope=0.01, makeup=0.1, attack=0.02, release=0.02)
    op, scale = mod.build_operator(mod.BLIND_DRC, cfg, "box", blind_drc=kw(*t, "--drc_makeup_db", "6", "--drc_fit", "makeup", cfg=cfg))
    assert isinstance(op, P.BlindDynamicRangeOperator) and scale == 1 and op.true_params["makeup_db"] == 6.0 and op.fit == ("makeup",)
    assert op.lr == (0.0, 0.0, 0.1, 0.0, 0.0) and op.noiser is not None and op.sample_rate == cfg.data.sample_rate
    with pytest.raises(ValueError):
        mod.build_operator(mod.BLIND_DRC, cfg, "box")
    args = mod.parse_args([*t, "--track_overlap_s", "1.28"])                    # track mode is allowed
    assert args.track_overlap_s == 1.28 and mod.spectral_boxes(args) is None and mod.separation_stems(args) is None
