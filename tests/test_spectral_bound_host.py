"""CPU: the float64 model of tests/spectral_cases.py equals torch.stft + autograd in float64 (the reference's own operator), the fp32
emulation of either route stays inside the element-wise bound on every element of every case, every mutant leaves it, the ambiguity
cap holds, and the refusal predicates the GPU file relies on say what csrc/audio_api.hip documents.

Figures of the last run (largest error / bound per output kind, `-s` prints them):
    fused emulation   mel 0.26   loss 0.038   dwav 0.0016       dense emulation   mel 0.26   dwav 0.0047   mag 0.053   dmag 0.00098
    weakest mutant    flo_late, 31 (fhi_short 33, ola_no_right_candidate 47, no_right_override 108)
    unseparated       c10_rounded reaches 0.018 (see spectral_cases)
    largest ambiguous share 0.26 % (cap 1 %)"""
import math

import numpy as np
import pytest
import torch

from tests import spectral_cases as S

IDS = [c.name for c in S.CASES]


def _torch_truth(c, i, dmag=None):
    """the chain with torch.stft + autograd, float64 -> (mel, loss or None, dwav, |X|)"""
    L, N = c.L, c.n_fft
    w = torch.from_numpy(i.wav[:, :L].astype(np.float64)).requires_grad_(True)
    y = w
    if i.mask is not None:                                  # the model's one fp32 product: same value, the mask as its derivative
        y = w * torch.from_numpy(i.mask.astype(np.float64))
        y = y + (torch.from_numpy((i.wav[:, :L] * i.mask[None]).astype(np.float64)) - y).detach()
    if i.thr is not None:
        cth = torch.from_numpy(i.thr.astype(np.float64))[:, None]
        y = torch.maximum(torch.minimum(y, cth), -cth)
    if i.z is not None:
        y = y + c.sigma * torch.from_numpy(i.z[:, :L].astype(np.float64))
    win = torch.hann_window(N, periodic=True, dtype=torch.float64) if c.hann else torch.ones(N, dtype=torch.float64)
    spec = torch.stft(y, N, c.hop, N, window=win, center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    mag = spec.abs()
    if dmag is not None:
        (g,) = torch.autograd.grad((mag * torch.from_numpy(dmag.astype(np.float64))).sum(), w)
        return None, None, g.numpy(), mag.detach().numpy()
    p = mag ** 2 if c.power2 else mag
    if i.zmag is not None:
        p = p + c.sigma * torch.from_numpy(i.zmag.astype(np.float64))
    v = torch.einsum("bkt,km->btm", p, torch.from_numpy(i.fb.astype(np.float64)))
    o = 10.0 * torch.log10(torch.clamp(v, min=S.FLOOR)) if c.to_db else v
    o = torch.clamp(o, c.lo, c.hi)
    if i.dmel is not None:
        (g,) = torch.autograd.grad((o * torch.from_numpy(i.dmel.astype(np.float64))).sum(), w)
        return o.detach().numpy(), None, g.numpy(), None
    loss = torch.linalg.vector_norm((torch.from_numpy(i.ref.astype(np.float64)) - o).flatten(1), dim=1)
    (g,) = torch.autograd.grad(loss.sum(), w)
    return o.detach().numpy(), loss.detach().numpy(), c.gscale * g.numpy(), None


def _close(a, b, what):
    scale = max(float(np.abs(b).max()), 1e-30)
    assert float(np.abs(a - b).max()) <= 1e-9 * scale, (what, float(np.abs(a - b).max()), scale)


@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_model_equals_torch_stft_float64(c):
    i = S.inputs(c)
    r = S.model(c, i)
    o, loss, g, _ = _torch_truth(c, i)
    _close(r.o, o, "mel")
    _close(r.dwav, g, "dwav")
    if loss is not None:
        _close(r.loss, loss, "loss")
    if c.route == "dense":
        rm = S.model(c, i, dmag=i.dmag)
        _, _, gm, mag = _torch_truth(c, i, dmag=i.dmag)
        _close(rm.absX.transpose(0, 2, 1), mag, "mag")
        _close(rm.dwav, gm, "dmag -> dwav")


_WORST = {}


@pytest.mark.parametrize("c", S.CASES, ids=IDS)
def test_emulation_inside_bound_and_ambiguity_cap(c):
    out, q = S.run_case(c)
    for kind, ratio in out.items():
        key = (c.route, kind)
        _WORST[key] = max(_WORST.get(key, 0.0), ratio)
        assert ratio <= 1.0, (c.name, kind, ratio)
    assert q.share <= S.AMBIG_CAP, (c.name, q.share)
    if c.lo == S.NEG and c.hi == S.POS:
        assert q.share == 0.0, (c.name, q.share)
    _WORST["share"] = max(_WORST.get("share", 0.0), q.share)
    r = S.model(c, S.inputs(c), forward_only=True)
    if c.to_db and c.lo > S.NEG and c.route == "fused":     # the clamped variant: both sides of both limits are populated
        below, above = float((r.o_raw < c.lo).mean()), float((r.o_raw > c.hi).mean())
        assert below > 0.02 and above > 0.02 and below + above < 0.9, (c.name, below, above)
    if S.inputs(c).thr is not None:
        inside = (np.abs(r.ym) <= S.inputs(c).thr[:, None]).mean(1)
        assert np.all((inside >= 0.05) & (inside <= 0.95)), (c.name, inside)
    print(f"\n{c.name}: " + " ".join(f"{k} {v:.2e}" for k, v in out.items()) + f" ambiguous {q.share:.4f}")


def test_worst_ratios_are_reported():
    """runs after the cases above (file order): prints the largest emulation / bound ratio per route and output kind"""
    print("\n" + "  ".join(f"{k}: {v:.3g}" for k, v in sorted(_WORST.items(), key=str)))


_WEAKEST = {}


@pytest.mark.parametrize("name", sorted(S.MUTANTS))
def test_every_mutant_leaves_the_bound(name):
    where, cases = S.MUTANTS[name]
    best = 0.0
    for cn in cases:
        out, _ = S.run_case(S.CASE[cn], name, where)
        best = max(best, max(out.values()))
    _WEAKEST[name] = best
    print(f"\nmutant {name}: {best:.3g}")
    assert best > 1.0, (name, best)


def test_weakest_mutant_is_reported_and_unseparated_ones_are_recorded():
    if _WEAKEST:
        name = min(_WEAKEST, key=_WEAKEST.get)
        print(f"\nweakest mutant: {name} at {_WEAKEST[name]:.3g}")
    for name, (where, cases) in S.UNSEPARATED.items():       # recorded, not asserted to leave: see the module docstring of spectral_cases
        best = max(max(S.run_case(S.CASE[cn], name, where)[0].values()) for cn in cases)
        print(f"unseparated mutant {name}: {best:.3g}")
        assert math.isfinite(best)


def test_case_table_covers_what_it_claims():
    fused = [c for c in S.CASES if c.route == "fused"]
    dense = [c for c in S.CASES if c.route == "dense"]
    assert 40 <= len(S.CASES) <= 60 and all(c.why for c in S.CASES)
    assert {c.L for c in fused} == {2048, 2049, 2207, 2560, 2561, 3361}
    assert {160, 480, 137, 1024, 1400} <= {c.hop for c in fused}
    for hop in (160, 480, 137, 1024, 1400):                 # every hop with every transform variant or length class it can meet
        assert len({c.L for c in fused if c.hop == hop}) >= 3, hop
    assert {c.mask for c in fused} == {None, "left", "right", "long", "frac"}
    assert any(c.shared_ref for c in fused) and any(c.cot and c.bank == "slaney" and c.hop == 480 for c in fused)
    assert {c.noise for c in fused} == {None, "sample", "mag"} and any(c.thr for c in fused) and any(c.gscale != 1.0 for c in fused)
    assert any(c.Lfull > c.L and c.stride > c.Lfull for c in fused)
    assert {c.n_fft for c in dense} == {64, 96, 256, 1024} and {16, 25, 100} <= {c.hop for c in dense}
    for n in (64, 96, 256):
        assert {c.L for c in dense if c.n_fft == n and not c.offset} == {n // 2 + 1, n, 3 * n + 7}, n
    assert {513, 1600, 2047} <= {c.L for c in dense if c.n_fft == 1024}
    assert any(c.stride % 2 for c in dense) and any((c.B * (1 + c.L // c.hop)) % 64 for c in dense) and any(c.offset == 1 for c in dense)
    for c in fused:                                         # a hole "longer than 1024 + hop" zeroes whole frames
        if c.mask == "long":
            i = S.inputs(c)
            assert (np.abs(S.model(c, i, forward_only=True).xw).sum(-1) == 0).any(), c.name


def test_zeroed_frames_and_uncovered_samples_are_exact_in_the_model():
    c = S.CASE["f3361_h160_dbc_hole"]
    i = S.inputs(c)
    r = S.model(c, i)
    q = S.bound(c, i, r)
    dead = np.abs(r.xw).sum(-1) == 0
    assert dead.any() and np.all(r.o_raw[dead] == -100.0) and not q.ambiguous[dead].any()
    assert np.all(r.dwav[:, i.mask == 0] == 0) and np.all(q.dwav[:, i.mask == 0] == 0)
    c = S.CASE["f3361_h1400_db"]
    r = S.model(c, S.inputs(c))
    assert (r.count == 0).any() and np.all(r.dwav[:, r.count == 0] == 0)
    assert np.all(S.bound(c, S.inputs(c), r).dwav[:, r.count == 0] == 0)


def test_refusal_predicates():
    assert S.fused_route(1024, 2048) and not S.fused_route(1024, 2047) and not S.fused_route(256, 4096)
    assert not S.refuses_transform(1024, 513) and S.refuses_transform(1024, 512) and S.refuses_transform(64, 32)
    assert S.refuses_guidance(1024, 2047, True, False, None)             # fused needs L >= 2048
    assert S.refuses_guidance(1024, 2048, True, True, None)              # magnitude-domain noise only with the magnitude transform
    assert not S.refuses_guidance(1024, 2048, False, True, None)
    assert S.refuses_guidance(1024, 2048, True, False, 2047)             # noise row stride >= L
    assert not S.refuses_guidance(1024, 2048, True, False, 2048)
    for c in S.CASES:
        assert not S.refuses_transform(c.n_fft, c.L), c.name
