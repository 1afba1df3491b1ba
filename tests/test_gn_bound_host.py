"""CPU: the float64 model, the element-wise bound and the case table of tests/gn_cases.py are validated from the reference alone, for
both activation types, so that the tolerance of tests/test_gpu_gn_elementwise.py is never fitted to a kernel:
  - the model agrees with torch's own float64 group_norm (+ silu) and its autograd;
  - an fp32 emulation of the documented arithmetic (one-pass chunk / slot sums Chan-combined in two sweeps, the register plan's two
    passes, scale / shift, the affine + SiLU, the 16-bit store, the backward sums with rstd applied afterwards) stays inside half the
    bound -- for 16-bit outputs half of what the bound leaves beside the one unavoidable output rounding (gn_cases docstring);
  - every mutant of the reference leaves the bound in at least one case;
  - outside the structure families the bound of y and dx is sharp: what is not the output rounding exceeds it in <= 10 % of the elements;
  - the table reaches every plan of the mirror at least twice, every tail of the 4-deep loops and a chunk shorter than the rows in flight."""
import pytest
import torch
import torch.nn.functional as F

from tests import gn_cases as N

ADTS = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
BY_NAME = {c.name: c for c in N.CASES}


def _tape(r):
    """the forward's tape as the backward reads it: fp32 values"""
    f = lambda t: t.float().double()
    return f(r.mean), f(r.rstd), f(r.scale), f(r.shift)


def _within(got, ref, lim, what):
    err = (got - ref).abs()
    ok = err <= lim
    worst = (err / lim.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} elements outside, worst err / limit {worst:.3f}"
    return worst


def test_model_is_torch_group_norm_and_its_autograd():
    g = torch.Generator().manual_seed(3)
    B, P, C, G, eps = 2, 37, 32, 4, 1e-5
    x = torch.randn(B, P, C, generator=g, dtype=torch.float64) * 1.7 + 0.6
    gamma, beta = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    dy, add = torch.randn(B, P, C, generator=g, dtype=torch.float64), torch.randn(B, P, C, generator=g, dtype=torch.float64)
    for silu in (0, 1):
        r = N.forward(x, gamma, beta, G, eps, silu)
        xr = x.clone().requires_grad_(True)
        yr = F.group_norm(xr.transpose(1, 2), G, gamma, beta, eps).transpose(1, 2)
        if silu:
            yr = F.silu(yr)
        assert (r.y - yr.detach()).abs().max().item() < 1e-12
        (gref,) = torch.autograd.grad((yr * dy).sum(), xr)
        b = N.backward(x, dy, add, r.mean, r.rstd, r.scale, r.shift, G, silu)
        assert (b.dx - (gref + add)).abs().max().item() < 1e-12
        # the slot sums are sums of the same terms
        (s, _), (q, _) = N.forward_slots(x, 16)
        assert (s.sum(1).view(B, G, -1).sum(2) / (P * C // G) - r.mean).abs().max().item() < 1e-12
        (t1, _), (t2, _) = N.backward_slots(x, dy, r.scale, r.shift, b, silu, 16)
        assert (t1.sum(1).view(B, G, -1).sum(2) / (P * C // G) - b.c1).abs().max().item() < 1e-12
        assert q.shape == t2.shape == (B, 3, C // 4)


def test_case_table_reaches_every_plan_and_tail():
    count, left, short = {}, {}, {}
    for c in N.CASES:
        count[c.plan] = count.get(c.plan, 0) + 1
        if c.plan != "register":
            lf, sh = N.tails(c.P, c.rpb, c.nchunk, c.ppb)
            left.setdefault(c.plan, set()).update(lf)
            short[c.plan] = short.get(c.plan, False) or sh
    assert set(count) == {"register", "fused", "three"} and min(count.values()) >= 2, count
    for pl in ("fused", "three"):
        assert left[pl] >= {1, 2, 3} and short[pl], (pl, left[pl], short[pl])
    for nm, want in (("fused-tail1", {1}), ("fused-tail2", {2}), ("fused-tail3", {3}), ("three-tail1", {1}), ("three-tail2", {2}), ("three-tail3", {3})):
        c = BY_NAME[nm]
        assert c.plan == nm.split("-")[0] and c.nchunk > 1 and N.tails(c.P, c.rpb, c.nchunk, c.ppb)[0] == want, nm
    c = BY_NAME["fused-short"]
    assert c.plan == "fused" and N.tails(c.P, c.rpb, c.nchunk, c.ppb)[1]
    # the thresholds: both sides of 512 and 8192 pixels and of 4096 register units; all 32 finalize iterations; the prologue's limits
    assert BY_NAME["reg-4096units"].plan == "register" and BY_NAME["three-4097units"].plan == "three"
    assert BY_NAME["three-p511"].plan == "three" and BY_NAME["fused-p512"].plan == "fused"
    assert BY_NAME["fused-32x64"].plan == "fused" and BY_NAME["three-p8193"].plan == "three"
    assert BY_NAME["three-512chunks"].nchunk == 512 and BY_NAME["fused-32x64"].nchunk == 32 and BY_NAME["fused-30chunks"].nchunk == 30
    assert BY_NAME["reg-stats-only"].plan == "register" and BY_NAME["three-g2-stats-only"].plan == "three"
    assert {c.family for c in N.CASES} == {"plain", "const", "near", "off4", "off16", "gamma30", "subn"}
    assert {c.C // c.G for c in N.CASES} >= {1, 2, 3, 4, 8, 20, 64, 256} and {c.G for c in N.CASES} >= {1, 2, 4, 8, 32, 64}


@pytest.mark.parametrize("adt", ADTS, ids=IDS)
@pytest.mark.parametrize("case", N.CASES, ids=repr)
def test_emulation_stays_inside_half_the_bound_and_the_bound_is_sharp(case, adt):
    c, d = case, case.data(adt)
    r = N.forward(d.x, d.gamma, d.beta, c.G, c.eps, c.silu, with_y=c.with_y)
    b = N.forward_bound(d.x, d.gamma, d.beta, c.G, c.eps, c.silu, r, c.d, c.two_pass, adt, with_y=c.with_y)
    e = N.emulate_forward(d.x, d.gamma, d.beta, c.G, c.eps, c.silu, adt, c.plan, ppb=c.ppb, with_y=c.with_y)
    w = {k: _within(getattr(e, k), getattr(r, k), N.emu_limit(getattr(b, k)), f"{c.name} {k}") for k in ("mean", "rstd", "scale", "shift")}
    if c.with_y:
        w["y"] = _within(e.y, r.y, N.emu_limit(b.y, b.y_round), f"{c.name} y")
        fr = N.sharp_fraction(b.y, b.y_round)
        print(f"{c.name}: y bound exceeds two roundings in {fr:.3f} of the elements")
        assert c.structure or fr <= 0.10, fr
    mean, rstd, scale, shift = _tape(r)
    for silu, with_add in c.bwd:
        add = d.add if with_add else None
        m = N.backward(d.x, d.dy, add, mean, rstd, scale, shift, c.G, silu)
        bb = N.backward_bound(d.x, d.dy, add, mean, rstd, scale, shift, c.G, silu, m, c.bwd_d, adt)
        eb = N.emulate_backward(d.x, d.dy, add, mean, rstd, scale, shift, c.G, silu, adt, c.bwd_ppb)
        tag = f"{c.name} silu {silu} add {int(with_add)}"
        w[f"k0/{silu}{int(with_add)}"] = _within(eb.k0, m.k0, N.emu_limit(bb.k0), tag + " k0")
        w[f"k1/{silu}{int(with_add)}"] = _within(eb.k1, m.k1, N.emu_limit(bb.k1), tag + " k1")
        w[f"dx/{silu}{int(with_add)}"] = _within(eb.dx, m.dx, N.emu_limit(bb.dx, bb.dx_round), tag + " dx")
        fr = N.sharp_fraction(bb.dx, bb.dx_round)
        assert c.structure or fr <= 0.10, (tag, fr)
    print(c.name, c.plan, "emulation err / limit:", "  ".join(f"{k} {v:.2f}" for k, v in w.items()))


def _producer_like(name, B, P, C, adt):
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    return (0.7 + 1.8 * torch.randn(B, P, C, generator=g, dtype=torch.float64)).to(adt).double(), \
        (1.0 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64)).float().double(), (0.2 * torch.randn(C, generator=g, dtype=torch.float64)).float().double()


@pytest.mark.parametrize("adt", ADTS, ids=IDS)
@pytest.mark.parametrize("entry", N.PRODUCER + [("prod-seam", 0, 3, 1000, 64, (64, 96), 8, 0)], ids=lambda e: e[0])
def test_emulation_of_the_slot_combine(entry, adt):
    """tensors shaped like the producer cases (the GPU test takes them from a GEMM): slot sums per quad, one-pass M2 per (slot, quad) item"""
    name, _, B, P, _, Cs, G, silu = entry
    srcs = Cs if isinstance(Cs, tuple) else (Cs,)
    C = sum(srcs)
    x, gamma, beta = _producer_like(name, B, P, C, adt)
    regions, emu_regions, c0 = [], [], 0
    for cn in srcs:
        regions.append((N.GN_SLOT, P, cn // 4))
        emu_regions.append((N.GN_SLOT, c0, cn))
        c0 += cn
    pl = N.parts_plan(P, C, True, regions)
    ns, cpg = N.cdiv(P, N.GN_SLOT), C // G
    d = N.adds(pl, P, C, G, regions=[(N.GN_SLOT, ns, N.cdiv(cpg, 4)) for _ in srcs])
    r = N.forward(x, gamma, beta, G, 1e-5, silu)
    b = N.forward_bound(x, gamma, beta, G, 1e-5, silu, r, d, False, adt)
    e = N.emulate_forward(x, gamma, beta, G, 1e-5, silu, adt, pl, regions=emu_regions)
    w = {k: _within(getattr(e, k), getattr(r, k), N.emu_limit(getattr(b, k)), f"{name} {k}") for k in ("mean", "rstd", "scale", "shift")}
    w["y"] = _within(e.y, r.y, N.emu_limit(b.y, b.y_round), f"{name} y")
    fr = N.sharp_fraction(b.y, b.y_round)
    assert fr <= 0.10, fr
    # the slot sums themselves, as fp32 sums of the stored values
    (s, sb), (q, qb) = N.forward_slots(x, N.GN_SLOT)
    es, _ = N._chunk_sums(x.float(), N.GN_SLOT, C // 4)
    eq, _ = N._chunk_sums(x.float() * x.float(), N.GN_SLOT, C // 4)
    w["sum"], w["sumsq"] = _within(es.double(), s, sb / 2, f"{name} slot sums"), _within(eq.double(), q, qb / 2, f"{name} slot sums of squares")
    print(name, pl, f"d {d} sharp {fr:.3f}", "  ".join(f"{k} {v:.2f}" for k, v in w.items()))


MUTANT_CASES = ["reg-p1", "three-cpg3", "three-tail1", "fused-ragged", "register-const-eps6", "three-subn", "fused-gamma30"]


@pytest.mark.parametrize("adt", ADTS, ids=IDS)
def test_every_mutant_of_the_reference_leaves_the_bound(adt):
    caught = {("fwd", m): [] for m in N.FWD_MUTANTS}
    caught.update({("bwd", m): [] for m in N.BWD_MUTANTS})
    for nm in MUTANT_CASES:
        c = BY_NAME[nm]
        d = c.data(adt)
        r = N.forward(d.x, d.gamma, d.beta, c.G, c.eps, c.silu)
        b = N.forward_bound(d.x, d.gamma, d.beta, c.G, c.eps, c.silu, r, c.d, c.two_pass, adt)
        for m in N.FWD_MUTANTS:
            mr = N.forward(d.x, d.gamma, d.beta, c.G, c.eps, c.silu, mut=m)
            out = [k for k in ("mean", "rstd", "scale", "shift", "y") if not bool(((getattr(mr, k) - getattr(r, k)).abs() <= getattr(b, k)).all())]
            if out:
                caught[("fwd", m)].append((nm, out))
        mean, rstd, scale, shift = _tape(r)
        ref = N.backward(d.x, d.dy, d.add, mean, rstd, scale, shift, c.G, 1)
        bb = N.backward_bound(d.x, d.dy, d.add, mean, rstd, scale, shift, c.G, 1, ref, c.bwd_d, adt)
        for m in N.BWD_MUTANTS:
            mr = N.backward(d.x, d.dy, d.add, mean, rstd, scale, shift, c.G, 1, mut=m)
            out = [k for k in ("k0", "k1", "dx") if not bool(((getattr(mr, k) - getattr(ref, k)).abs() <= getattr(bb, k)).all())]
            if out:
                caught[("bwd", m)].append((nm, out))
    for k, v in caught.items():
        print(k, v)
    missed = [k for k, v in caught.items() if not v]
    assert not missed, f"mutants that stay inside the bound everywhere: {missed}"
    # a mutant that only moves the count of a slot shows where the image is no multiple of the slot rows, and nowhere else
    assert all(BY_NAME[nm].P % N.GN_SLOT for nm, _ in caught[("fwd", "last_slot_full")])
