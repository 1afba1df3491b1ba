"""CPU: the float64 models, the element-wise bounds and the case tables of tests/htsat_cases.py are validated without a GPU, for both
activation types, so that no tolerance of tests/test_gpu_htsat_elementwise.py is fitted to a kernel:
  - the models agree with transformers' own CLAP modules in float64 (ClapAudioLayer shifted and unshifted on a non-square grid,
    ClapAudioPatchMerging, BatchNorm + reshape_mel2img + ClapAudioPatchEmbed) to 1e-10 relative;
  - an fp32 emulation of each kernel's documented arithmetic stays inside half the bound (for 16-bit outputs: half of what the bound
    leaves beside the one output rounding);
  - the bounds are sharp: the fp32 term exceeds eps |ref| in at most 10 % of the elements of a 16-bit forward output and 30 % of a
    16-bit backward output (htsat_cases docstring: what is exempt and why);
  - every mutant of the models leaves the bound in the case named for it."""
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import htsat_cases as N

ADTS = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
FWD_CAP, BWD_CAP = 0.10, 0.30


def _within(got, ref, lim, what):
    err = (got - ref).abs()
    ok = err <= lim
    worst = (err / lim.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} elements outside, worst err / limit {worst:.3f}"
    return worst


def _killed(mutant, ref, bound, what):
    out = (mutant - ref).abs() > bound
    assert bool(out.any()), f"mutant {what} stays inside the bound"
    return int(out.sum())


def _median_rel(bound, ref):
    return (bound / ref.abs().clamp_min(1e-300)).median().item()


def _by_name(cases):
    return {c.name: c for c in cases}


# ===================================================================================================================== LayerNorm rows
def _ln_variants(c):
    """(dy is fp32, add present) of the backward: both dy types, add present and absent (a patch merging takes no add)"""
    return [(False, False), (True, False)] + ([] if c.merge else [(False, True), (True, True)])


def _keep(c, t):
    """rows (or, flat, their elements) outside the exempt rows"""
    if not c.exempt_rows:
        return t
    m = torch.ones(t.shape[0], dtype=torch.bool)
    m[c.exempt_rows] = False
    return t[m]


@pytest.mark.parametrize("adt", ADTS, ids=IDS)
@pytest.mark.parametrize("case", N.LN_CASES, ids=repr)
def test_layernorm_rows_emulation_and_sharpness(case, adt):
    c, d = case, case.data(adt)
    xr = c.rows_of(d.x)
    ref = c.forward(d)
    for o in [adt] + ([None] if c.out32 else []):
        b = c.forward_bound(d, ref, o)
        _within(N.ln_emulate_forward(xr, d.gamma, d.beta, c.eps, o), ref, N.emu_limit(b, ref, o), f"{c} y {o}")
        if o is not None:
            assert N.sharp_fraction(_keep(c, b), _keep(c, ref), o) <= FWD_CAP, (c, N.sharp_fraction(_keep(c, b), _keep(c, ref), o))
        else:
            print(f"{c} y fp32: median bound / |ref| {_median_rel(b, ref):.2e}")
    idx = N.ln_source_index(d.x.numel(), c.C, c.merge, c.H, c.W, c.rows)
    for dy32, with_add in _ln_variants(c):
        dy, add = (d.dy32 if dy32 else d.dy), (d.add if with_add else None)
        ref = c.backward(d, dy, add)
        b, written = c.backward_bound(d, dy, add, ref, adt)
        assert bool((ref[~written] == 0).all())
        emu = N.ln_emulate_backward(xr, dy, None if add is None else add[idx], d.gamma, c.eps, adt)
        _within(emu, ref[idx], N.emu_limit(b[idx], ref[idx], adt), f"{c} dx dy32 {dy32} add {with_add}")
        sf = N.sharp_fraction(_keep(c, b[idx]), _keep(c, ref[idx]), adt)
        assert sf <= BWD_CAP, (c, dy32, with_add, sf)


def test_layernorm_table_reaches_the_documented_geometry():
    by = _by_name(N.LN_CASES)
    assert N.ln_geom(8) == (1, 256, 1) and N.ln_geom(96) == (16, 16, 12) and N.ln_geom(768) == (64, 4, 96) and N.ln_geom(192) == (32, 8, 24)
    assert N.ln_geom(1536) == (64, 4, 192) and by["ln-c1536-r5"].Cw == N.LN_MAX_WIDTH == by["ln-merge-c384-2x2-r5"].Cw
    for C in (8, 96, 768):
        rpb = N.ln_geom(C)[1]
        rows = sorted(c.rows for c in N.LN_CASES if c.C == C and not c.merge and c.family == "plain")
        assert rows[0] == 1 and rows[1] == rpb + 1 and rows[2] % rpb not in (0, 1), (C, rows)
    assert by["ln-merge-c48-4x6-r9"].tokens == 48 and by["ln-merge-c48-4x6-r9"].rows == N.ln_geom(192)[1] + 1
    assert {c.family for c in N.LN_CASES} == {"plain", "offset", "const"}
    d = by["ln-c96-offset"].data(torch.float16)
    xr = by["ln-c96-offset"].rows_of(d.x)
    assert float((xr.mean(1).abs() / xr.std(1)).min()) > 20.0


@pytest.mark.parametrize("adt", ADTS, ids=IDS)
def test_layernorm_mutants_are_killed(adt):
    by = _by_name(N.LN_CASES)
    for mut, name in N.LN_MUTANTS.items():
        c = by[name]
        d = c.data(adt)
        ref = c.forward(d)
        _killed(c.forward(d, mut), ref, c.forward_bound(d, ref, adt), f"{mut} on {name} (forward)")
    for mut, name in N.LN_BWD_MUTANTS.items():
        c = by[name]
        d = c.data(adt)
        ref = c.backward(d, d.dy, None if c.merge else d.add)
        b, _ = c.backward_bound(d, d.dy, None if c.merge else d.add, ref, adt)
        _killed(c.backward(d, d.dy, None if c.merge else d.add, mut), ref, b, f"{mut} on {name} (backward)")


# ================================================================================================================================ GELU
@pytest.mark.parametrize("adt", ADTS, ids=IDS)
@pytest.mark.parametrize("case", N.GELU_CASES, ids=repr)
def test_gelu_emulation_and_sharpness(case, adt):
    d = case.data(adt)
    ref = N.gelu(d.u)
    b = N.out_bound(N.gelu_forward_term(d.u), ref, adt)
    _within(N.gelu_emulate_forward(d.u, adt), ref, N.emu_limit(b, ref, adt), f"{case} y")
    gref = N.gelu_backward(d.u, d.dy)
    gb = N.out_bound(N.gelu_backward_term(d.u, d.dy, gref), gref, adt)
    _within(N.gelu_emulate_backward(d.u, d.dy, adt), gref, N.emu_limit(gb, gref, adt), f"{case} du")
    if not case.exempt:
        assert N.sharp_fraction(b, ref, adt) <= FWD_CAP, N.sharp_fraction(b, ref, adt)
        assert N.sharp_fraction(gb, gref, adt) <= BWD_CAP, N.sharp_fraction(gb, gref, adt)
    # the documented cancellation: at u = -4 the bound's absolute term is about one 16-bit ulp of the result (fp16)
    u = torch.tensor([-4.0], dtype=torch.float64)
    assert 0.5 * 4.0 * N.ERF_ULP * N.ULP <= float(N.gelu_forward_term(u)) <= 4 * 0.5 * 4.0 * N.ERF_ULP * N.ULP


@pytest.mark.parametrize("adt", ADTS, ids=IDS)
def test_gelu_tanh_mutant_is_killed(adt):
    case = _by_name(N.GELU_CASES)[N.GELU_MUTANTS["tanh"]]
    d = case.data(adt)
    ref = N.gelu(d.u)
    _killed(N.gelu(d.u, "tanh"), ref, N.out_bound(N.gelu_forward_term(d.u), ref, adt), "tanh-GELU (forward)")
    gref = N.gelu_backward(d.u, d.dy)
    _killed(N.gelu_backward(d.u, d.dy, "tanh"), gref, N.out_bound(N.gelu_backward_term(d.u, d.dy, gref), gref, adt), "tanh-GELU (backward)")


# ==================================================================================================================== window attention
@pytest.mark.parametrize("adt", ADTS, ids=IDS)
@pytest.mark.parametrize("case", N.ATTN_CASES, ids=repr)
def test_window_attention_emulation_and_sharpness(case, adt):
    c, d = case, case.data(adt)
    ref = N.win_attn(d.qkv, d.table, *c.geom)
    b = N.win_attn_forward_bound(d.qkv, d.table, ref, *c.geom, adt)
    gref = N.win_attn_backward(d.qkv, d.dout, d.table, *c.geom)
    gb = N.win_attn_backward_bound(d.qkv, d.dout, d.table, gref, *c.geom, adt)
    out, dqkv = N.win_attn_emulate(d.qkv, d.dout, d.table, *c.geom, adt)
    _within(out, ref, N.emu_limit(b, ref, adt), f"{c} out")
    _within(dqkv, gref, N.emu_limit(gb, gref, adt), f"{c} dqkv")
    sf = N.sharp_fraction(b, ref, adt)
    assert sf <= FWD_CAP, (c, sf)
    g3, b3 = gref.view(c.B, c.H * c.W, 3, c.C), gb.view(c.B, c.H * c.W, 3, c.C)
    for j, nm in enumerate(("dq", "dk", "dv")):
        sf = N.sharp_fraction(b3[:, :, j], g3[:, :, j], adt)
        print(f"{c} {nm}: share of unsharp elements {sf:.3f}")
        assert sf <= BWD_CAP, (c, nm, sf)


def test_window_attention_table_has_what_it_is_there_for():
    by = _by_name(N.ATTN_CASES)
    c = by["attn-16x16-shift"]
    lab = N.region_labels(c.H, c.W, c.shift)
    assert sorted(lab.unique().tolist()) == list(range(9))                          # all nine regions occur
    assert {(c.H, c.W) for c in N.ATTN_CASES} >= {(8, 8), (16, 16), (16, 24), (24, 16)}
    # the competitive case: masked logits of about -40 and -3 beside the row maximum
    c = by["attn-competitive"]
    d = c.data(torch.float16)
    q, k, v, bias, masked, sh = N._win_split(d.qkv, d.table, *c.geom)
    s = (q * N.HD ** -0.5) @ k.transpose(-1, -2)
    top = torch.where(masked[None, :, None], s, torch.full((), -1e9, dtype=torch.float64)).flatten().topk(4).values
    assert 90.0 < float(top[0]) < 104.0 and any(50.0 < float(t) < 70.0 for t in top), top
    # the relative position index is transformers' own
    from transformers.models.clap.modeling_clap import ClapAudioSelfAttention
    att = ClapAudioSelfAttention(NS(attention_probs_dropout_prob=0.0, qkv_bias=True), 48, 2, 8)
    assert torch.equal(att.relative_position_index, N.rel_position_index())


@pytest.mark.parametrize("adt", ADTS, ids=IDS)
def test_window_attention_mutants_are_killed(adt):
    by = _by_name(N.ATTN_CASES)
    for mut, name in N.ATTN_MUTANTS.items():
        c = by[name]
        d = c.data(adt)
        ref = N.win_attn(d.qkv, d.table, *c.geom)
        _killed(N.win_attn(d.qkv, d.table, *c.geom, mut), ref, N.win_attn_forward_bound(d.qkv, d.table, ref, *c.geom, adt), f"{mut} on {name} (forward)")
        gref = N.win_attn_backward(d.qkv, d.dout, d.table, *c.geom)
        gb = N.win_attn_backward_bound(d.qkv, d.dout, d.table, gref, *c.geom, adt)
        _killed(N.win_attn_backward(d.qkv, d.dout, d.table, *c.geom, mut), gref, gb, f"{mut} on {name} (backward)")


# =============================================================================================================================== embed
@pytest.mark.parametrize("adt", ADTS, ids=IDS)
@pytest.mark.parametrize("case", N.EMBED_CASES, ids=repr)
def test_embed_emulation_and_sharpness(case, adt):
    c, d, cfg = case, case.data(adt), N.embed_config(case.E)
    ref = N.embed_forward(d.mel, d.P, cfg)
    b = N.embed_forward_bound(d.mel, d.P, cfg, ref, adt)
    dimg, dmel = N.embed_backward(d.mel, d.dtok, d.scale, d.P, cfg)
    b_dimg, b_dmel = N.embed_backward_bound(d.mel, d.dtok, d.scale, d.P, cfg, dimg, dmel)
    tok, e_dimg, e_dmel = N.embed_emulate(d.mel, d.dtok, d.scale, d.P, cfg, adt)
    _within(tok, ref, N.emu_limit(b, ref, adt), f"{c} tokens")
    _within(e_dimg, dimg, N.emu_limit(b_dimg), f"{c} dimg")
    _within(e_dmel, dmel, N.emu_limit(b_dmel), f"{c} dmel")
    sf = N.sharp_fraction(b, ref, adt)
    assert sf <= FWD_CAP, (c, sf)
    print(f"{c}: median bound / |ref| dimg {_median_rel(b_dimg, dimg):.2e}, dmel {_median_rel(b_dmel, dmel):.2e}")


def test_embed_table_and_taps():
    assert sorted({c.frames for c in N.EMBED_CASES}) == [2, 3, 100, 127, 128] and {c.E for c in N.EMBED_CASES} == {8, N.EMB_MAX}
    assert {c.with_scale for c in N.EMBED_CASES if c.E == 8} == {True, False} == {c.with_scale for c in N.EMBED_CASES if c.E == 128}
    idx, w = N.bicubic_taps(128, 128)
    assert torch.equal(idx[:, 1], torch.arange(128)) and torch.equal(w, torch.tensor([0.0, 1.0, 0.0, 0.0]).double().expand(128, 4))
    separated = 0
    for frames in (2, 3, 100, 127):
        idx, w = N.bicubic_taps(frames, 128)
        assert (w.sum(1) - 1).abs().max() < 1e-12 and int(idx.min()) == 0 and int(idx.max()) == frames - 1
        # the float32 rule, restated with numpy scalars: the index, its floor and the fraction are float32, the cubic is float64
        src = np.float32(frames - 1) / np.float32(127) * np.arange(128, dtype=np.float32)
        assert src.dtype == np.float32
        i0 = np.floor(src)
        fr = torch.from_numpy((src - i0).astype(np.float64))
        A = -0.75
        near = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
        far = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
        want_w = torch.stack([far(fr + 1), near(fr), near(1 - fr), far(2 - fr)], 1)
        want_idx = (torch.from_numpy(i0.astype(np.int64))[:, None] + torch.arange(-1, 3)).clamp(0, frames - 1)
        assert torch.equal(idx, want_idx) and (w - want_w).abs().max() < 1e-15
        w64 = N.bicubic_taps(frames, 128, index_dtype=torch.float64)[1]
        separated += int((w - w64).abs().max() > 1e-9)                              # a float64 index gives other weights
        # torch's own float32 bicubic stretch uses these taps
        x = torch.randn(1, 1, frames, 3)
        want = torch.nn.functional.interpolate(x, (128, 3), mode="bicubic", align_corners=True)[0, 0].double()
        got = N.stretch(x[0].double(), idx, w)[0]
        assert (got - want).abs().max() < 2e-6
    assert separated >= 2


@pytest.mark.parametrize("adt", ADTS, ids=IDS)
def test_embed_mutants_are_killed(adt):
    by = _by_name(N.EMBED_CASES)
    for mut, name in N.EMBED_MUTANTS.items():
        c = by[name]
        d, cfg = c.data(adt), N.embed_config(c.E)
        ref = N.embed_forward(d.mel, d.P, cfg)
        _killed(N.embed_forward(d.mel, d.P, cfg, mut=mut), ref, N.embed_forward_bound(d.mel, d.P, cfg, ref, adt), f"{mut} on {name} (tokens)")
        dimg, dmel = N.embed_backward(d.mel, d.dtok, d.scale, d.P, cfg)
        _, b_dmel = N.embed_backward_bound(d.mel, d.dtok, d.scale, d.P, cfg, dimg, dmel)
        _killed(N.embed_backward(d.mel, d.dtok, d.scale, d.P, cfg, mut)[1], dmel, b_dmel, f"{mut} on {name} (dmel)")


# ================================================================================================================================ Gram
@pytest.mark.parametrize("case", N.GRAM_CASES, ids=repr)
def test_gram_emulation(case):
    d = case.data()
    G, dF = N.gram(d.F), N.gram_backward(d.F, d.dG)
    bG, bdF = N.gram_bounds(d.F, d.dG)
    eG, edF = N.gram_emulate(d.F, d.dG)
    _within(eG, G, N.emu_limit(bG), f"{case} G")
    _within(edF, dF, N.emu_limit(bdF), f"{case} dF")
    assert (d.dG - d.dG.transpose(1, 2)).abs().max() > 0.1 or case.C == 1
    print(f"{case}: median bound / |ref| G {_median_rel(bG, G):.2e}, dF {_median_rel(bdF, dF):.2e}")


def test_gram_mutants_are_killed():
    by = _by_name(N.GRAM_CASES)
    for mut, name in N.GRAM_MUTANTS.items():
        d = by[name].data()
        bG, bdF = N.gram_bounds(d.F, d.dG)
        if mut == "gram_over_c":
            _killed(N.gram(d.F, mut), N.gram(d.F), bG, f"{mut} (forward)")
        _killed(N.gram_backward(d.F, d.dG, mut), N.gram_backward(d.F, d.dG), bdF, f"{mut} (backward)")


# ========================================================================================================= the models are the network
def _rel(a, b):
    return float((a.detach() - b.detach()).norm() / b.detach().norm())


def _randomise(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.endswith("relative_position_bias_table"):
                p.copy_(0.5 * torch.randn(p.shape, generator=g, dtype=torch.float64))
            elif "norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g, dtype=torch.float64))
            elif name.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64))
    return mod


@pytest.mark.parametrize("shift", [0, 4])
def test_model_is_transformers_swin_layer(shift):
    """ClapAudioLayer on a non-square 16 x 24 grid, heads of 24 channels: LayerNorm rows, window attention and GELU of this file composed
    with the module's own Linear weights, forward and input gradient"""
    from transformers import ClapAudioConfig
    from transformers.models.clap.modeling_clap import ClapAudioLayer
    H, W, heads = 16, 24, 2
    C = heads * N.HD
    cfg = ClapAudioConfig(window_size=8, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    layer = _randomise(ClapAudioLayer(cfg, C, (H, W), heads, 0.0, shift).double().eval(), 5)
    assert layer.shift_size == shift and layer.window_size == 8
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, H * W, C, generator=g, dtype=torch.float64, requires_grad=True)
    cot = torch.randn(2, H * W, C, generator=g, dtype=torch.float64)
    want = layer(x, (H, W))[0]
    (gwant,) = torch.autograd.grad((want * cot).sum(), x)

    def mine(x):
        lin = torch.nn.functional.linear
        sa, eps = layer.attention.self, cfg.layer_norm_eps
        y = N.ln_forward(x.reshape(-1, C), layer.layernorm_before.weight, layer.layernorm_before.bias, eps).view(x.shape)
        qkv = torch.cat([lin(y, m.weight, m.bias) for m in (sa.query, sa.key, sa.value)], -1)
        ao = N.win_attn(qkv, sa.relative_position_bias_table, 2, H, W, heads, shift)
        mid = x + lin(ao, layer.attention.output.dense.weight, layer.attention.output.dense.bias)
        y2 = N.ln_forward(mid.reshape(-1, C), layer.layernorm_after.weight, layer.layernorm_after.bias, eps).view(x.shape)
        u = lin(y2, layer.intermediate.dense.weight, layer.intermediate.dense.bias)
        return mid + lin(N.gelu(u), layer.output.dense.weight, layer.output.dense.bias)

    x2 = x.detach().clone().requires_grad_(True)
    got = mine(x2)
    (ggot,) = torch.autograd.grad((got * cot).sum(), x2)
    assert _rel(got.detach(), want.detach()) < 1e-10 and _rel(ggot, gwant) < 1e-10


def test_model_is_transformers_patch_merging():
    from transformers.models.clap.modeling_clap import ClapAudioPatchMerging
    B, H, W, C = 2, 4, 6, 48
    pm = _randomise(ClapAudioPatchMerging(C).double().eval(), 7)
    x = torch.randn(B, H * W, C, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    want = pm(x, (H, W))
    rows = N.ln_gather(x.reshape(-1), C, 1, H, W, B * (H // 2) * (W // 2))
    got = torch.nn.functional.linear(N.ln_forward(rows, pm.norm.weight, pm.norm.bias, pm.norm.eps), pm.reduction.weight).view(want.shape)
    assert _rel(got, want.detach()) < 1e-10


@pytest.mark.parametrize("frames", [3, 100, 128])
def test_model_is_transformers_input_stage(frames):
    """BatchNorm2d over the mel bins, ClapAudioEncoder.reshape_mel2img and ClapAudioPatchEmbed at the small configuration, in float64 (the
    source index of the stretch in float64 too, as torch computes it for a float64 tensor)"""
    from transformers import ClapAudioConfig
    from transformers.models.clap.modeling_clap import ClapAudioEncoder, ClapAudioPatchEmbed
    E = 8
    cfg, P = N.embed_config(E), N.embed_params(E)
    hf = ClapAudioConfig(spec_size=cfg.spec, num_mel_bins=cfg.bins, patch_embeds_hidden_size=E, patch_size=4, patch_stride=[4, 4])
    pe = ClapAudioPatchEmbed(hf).double().eval()
    bn = torch.nn.BatchNorm2d(cfg.bins).double().eval()
    with torch.no_grad():
        pe.proj.weight.copy_(P.Wp), pe.proj.bias.copy_(P.bp), pe.norm.weight.copy_(P.ln_g), pe.norm.bias.copy_(P.ln_b)
        bn.weight.copy_(P.bn_w), bn.bias.copy_(P.bn_b), bn.running_mean.copy_(P.bn_m), bn.running_var.copy_(P.bn_v)
    mel = N.EmbedCase(E, frames, True).data(torch.float16).mel.clone().requires_grad_(True)
    enc = NS(spec_size=cfg.spec, freq_ratio=cfg.spec // cfg.bins)
    x = bn(mel[:, None].transpose(1, 3)).transpose(1, 3)                       # ClapAudioEncoder.forward
    want = pe(ClapAudioEncoder.reshape_mel2img(enc, x))
    cot = torch.randn(want.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    (gwant,) = torch.autograd.grad((want * cot).sum(), mel)
    m2 = mel.detach().clone().requires_grad_(True)
    got = N.embed_forward(m2, P, cfg, index_dtype=torch.float64)
    (ggot,) = torch.autograd.grad((got * cot).sum(), m2)
    assert math.isclose(bn.eps, cfg.bn_eps) and math.isclose(pe.norm.eps, cfg.ln_eps)
    assert _rel(got.detach(), want.detach()) < 1e-10 and _rel(ggot, gwant) < 1e-10
