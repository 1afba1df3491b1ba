"""-m gpu: every kernel of the CLAP HTS-AT tower (csrc/htsat.hip) on its own, through the test hooks dmx_htsat_*_raw (and the public
dmx_gram_*), element by element against the float64 models of tests/htsat_cases.py on the same rounded inputs.  The bounds come from
the number formats and operation counts (htsat_cases docstring; validated on the CPU by tests/test_htsat_bound_host.py), never from a
kernel's output.  Every output buffer is pre-filled with a sentinel bit pattern and followed by a guard region; what a kernel must
not write (the guard, the tokens no row of a partial patch merging reads) has to keep it.  Each backward hook runs twice and has
to give the same bits (the tower promises no atomics).  The worst err / bound per kernel is printed at the end of the module."""
import ctypes as C

import pytest
import torch

from tests import htsat_cases as N

pytestmark = pytest.mark.gpu
SENT16, SENT32 = N.SENT16, N.SENT32
GUARD = 64
WORST = {}


def _L():
    from diffmusic_amd import _lib as L
    return L


def _adt():
    return _L().act_dtype()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _act(t):
    """float64 values of the activation type -> device tensor of that type"""
    return t.to(_adt()).cuda().contiguous()


def _f32(t):
    return t.float().cuda().contiguous() if t is not None else None


def _out16(n):
    return torch.full((n + GUARD,), SENT16, dtype=torch.int16, device="cuda")


def _out32(n):
    return torch.full((n + GUARD,), SENT32, dtype=torch.int32, device="cuda")


def _read16(buf, n, what):
    o = buf.cpu()
    assert bool((o[n:] == SENT16).all()), f"{what}: wrote behind the buffer"
    return o[:n]


def _read32(buf, n, what):
    o = buf.cpu()
    assert bool((o[n:] == SENT32).all()), f"{what}: wrote behind the buffer"
    return o[:n]


def _vals16(bits):
    return bits.contiguous().view(_adt()).double()


def _vals32(bits):
    return bits.contiguous().view(torch.float32).double()


def _run(rc, what):
    torch.cuda.synchronize()
    _L().check(rc, what)


def _refused(rc, what, match):
    L = _L()
    torch.cuda.synchronize()
    assert rc != 0, what
    assert L.lib().dmx_last_error(), what
    with pytest.raises(L.DmxError, match=match):
        L.check(rc, what)


def _check(kernel, what, got, ref, bound):
    assert bool(torch.isfinite(got).all()), what
    ratio = ((got - ref).abs() / bound.clamp_min(1e-300)).max().item() if got.numel() else 0.0
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    print(f"htsat elementwise: {kernel:<14} {what:<48} worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, (kernel, what, ratio, int(((got - ref).abs() > bound).sum()))


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for k in sorted(WORST):
        print(f"htsat elementwise: worst err / bound of {k:<14} {WORST[k]:.3f}")


# ===================================================================================================================== LayerNorm rows
def _ln_fwd(c, x, gamma, beta, out32, rows=None, C_=None, merge=None, H=None, W=None, n_out=None):
    rows, C_, merge = (c.rows if rows is None else rows), (c.C if C_ is None else C_), (c.merge if merge is None else merge)
    H, W = (c.H if H is None else H), (c.W if W is None else W)
    n = c.rows * c.Cw if n_out is None else n_out
    y = _out32(n) if out32 else _out16(n)
    rc = _L().lib().dmx_htsat_ln_rows_fwd_raw(_p(x), _p(y), _p(gamma), _p(beta), rows, C_, merge, H, W, c.eps, int(out32), _st())
    return rc, y, n


def _ln_bwd(c, x, dy, add, gamma, dy32, **over):
    a = dict(rows=c.rows, C=c.C, merge=c.merge, H=c.H, W=c.W)
    a.update(over)
    n = x.numel()
    dx = _out16(n)
    rc = _L().lib().dmx_htsat_ln_rows_bwd_raw(_p(x), _p(dy), _p(add), _p(dx), _p(gamma), a["rows"], a["C"], a["merge"], a["H"], a["W"], c.eps,
                                              int(dy32), _st())
    return rc, dx, n


@pytest.mark.parametrize("case", N.LN_CASES, ids=repr)
def test_layernorm_rows(case):
    c, adt = case, _adt()
    d = c.data(adt)
    x, gamma, beta = _act(d.x), _f32(d.gamma), _f32(d.beta)
    ref = c.forward(d)
    for out32 in [False] + ([True] if c.out32 else []):
        what = f"{c} y {'fp32' if out32 else '16-bit'}"
        rc, y, n = _ln_fwd(c, x, gamma, beta, out32)
        _run(rc, what)
        got = (_vals32(_read32(y, n, what)) if out32 else _vals16(_read16(y, n, what))).view(ref.shape)
        _check("ln_rows_fwd", what, got, ref, c.forward_bound(d, ref, None if out32 else adt))
    for dy32 in (False, True):
        for with_add in ([False] if c.merge else [False, True]):
            what = f"{c} dx dy {'fp32' if dy32 else '16-bit'}{' + add' if with_add else ''}"
            dyv, addv = (d.dy32 if dy32 else d.dy), (d.add if with_add else None)
            dy = _f32(dyv) if dy32 else _act(dyv)
            add = _act(addv) if with_add else None
            gref = c.backward(d, dyv, addv)
            bound, written = c.backward_bound(d, dyv, addv, gref, adt)
            rc, dx, n = _ln_bwd(c, x, dy, add, gamma, dy32)
            _run(rc, what)
            bits = _read16(dx, n, what)
            assert bool((bits[~written] == SENT16).all()), f"{what}: wrote a token no row reads"
            got = _vals16(bits)
            _check("ln_rows_bwd", what, got[written], gref[written], bound[written])
            rc, dx2, _ = _ln_bwd(c, x, dy, add, gamma, dy32)
            _run(rc, what)
            assert torch.equal(dx2, dx), what


def test_layernorm_rows_refusals():
    c = N.LnCase("refusal", 96, 4)
    x = _act(torch.zeros(4 * 1600, dtype=torch.float64))
    g = _f32(torch.ones(1600, dtype=torch.float64))
    for over, match in ((dict(C_=12), "multiple of 8"), (dict(C_=1544), "1536"), (dict(C_=392, merge=1, H=2, W=2, rows=1), "1536"),
                        (dict(rows=0), "rows"), (dict(C_=48, merge=1, H=3, W=6, rows=1), "even")):
        for out32 in (False, True):
            rc, y, n = _ln_fwd(c, x, g, g, out32, n_out=4 * 1600, **over)
            _refused(rc, f"ln forward {over}", match)
            assert bool(((_read32 if out32 else _read16)(y, n, "refused") == (SENT32 if out32 else SENT16)).all())
    dy = _act(torch.zeros(4 * 1600, dtype=torch.float64))
    for over, add, match in ((dict(C=12), None, "multiple of 8"), (dict(C=1544), None, "1536"), (dict(C=392, merge=1, H=2, W=2, rows=1), None, "1536"),
                             (dict(rows=0), None, "rows"), (dict(C=48, merge=1, H=4, W=6, rows=1), x, "merge with add")):
        for dy32 in (False, True):
            rc, dx, n = _ln_bwd(c, x, _f32(dy.double()) if dy32 else dy, add, g, dy32, **over)
            _refused(rc, f"ln backward {over}", match)
            assert bool((_read16(dx, n, "refused") == SENT16).all())


# ================================================================================================================================ GELU
@pytest.mark.parametrize("case", N.GELU_CASES, ids=repr)
def test_gelu(case):
    adt, lib = _adt(), _L().lib()
    d = case.data(adt)
    n = case.n8 * 8
    u, dy = _act(d.u), _act(d.dy)
    ref = N.gelu(d.u)
    y = _out16(n)
    _run(lib.dmx_htsat_gelu_fwd_raw(_p(u), _p(y), case.n8, _st()), f"{case} y")
    got = _vals16(_read16(y, n, "gelu y"))
    _check("gelu_fwd", f"{case} y", got, ref, N.out_bound(N.gelu_forward_term(d.u), ref, adt))
    zero = d.u == 0
    assert int(zero.sum()) >= 2 and bool(torch.signbit(d.u[zero]).any()) and not bool(torch.signbit(d.u[zero]).all())
    assert torch.equal(torch.signbit(got[zero]), torch.signbit(ref[zero])), f"{case}: gelu(+-0.0) lost the sign of zero"
    gref = N.gelu_backward(d.u, d.dy)
    gb = N.out_bound(N.gelu_backward_term(d.u, d.dy, gref), gref, adt)
    outs = []
    for run, in_place in enumerate((False, True, False)):                  # out of place twice: the same bits run to run
        du = _out16(n)
        if in_place:                                                       # the tower's own call: du == dy
            du[:n] = dy.view(torch.int16)
        rc = lib.dmx_htsat_gelu_bwd_raw(_p(u), _p(du) if in_place else _p(dy), _p(du), case.n8, _st())
        _run(rc, f"{case} du")
        bits = _read16(du, n, "gelu du")
        if run < 2:
            _check("gelu_bwd", f"{case} du {'in place' if in_place else 'out of place'}", _vals16(bits), gref, gb)
        outs.append(bits)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_gelu_refusals():
    lib = _L().lib()
    u, y = _act(torch.zeros(8, dtype=torch.float64)), _out16(8)
    _refused(lib.dmx_htsat_gelu_fwd_raw(_p(u), _p(y), 0, _st()), "gelu n8 0", "at least 1")
    _refused(lib.dmx_htsat_gelu_bwd_raw(_p(u), _p(u), _p(y), 0, _st()), "gelu backward n8 0", "at least 1")
    assert bool((y.cpu() == SENT16).all())


# ==================================================================================================================== window attention
@pytest.mark.parametrize("case", N.ATTN_CASES, ids=repr)
def test_window_attention(case):
    c, adt, lib = case, _adt(), _L().lib()
    d = c.data(adt)
    B, H, W, heads, shift = c.geom
    qkv, dout, table = _act(d.qkv), _act(d.dout), _f32(d.table)
    n = B * H * W * c.C
    ref = N.win_attn(d.qkv, d.table, *c.geom)
    out = _out16(n)
    _run(lib.dmx_htsat_win_attn_fwd_raw(_p(qkv), _p(out), _p(table), B, H, W, c.C, heads, shift, _st()), f"{c} out")
    got = _vals16(_read16(out, n, f"{c} out")).view(ref.shape)
    _check("win_attn_fwd", f"{c} out", got, ref, N.win_attn_forward_bound(d.qkv, d.table, ref, *c.geom, adt))
    gref = N.win_attn_backward(d.qkv, d.dout, d.table, *c.geom)
    gb = N.win_attn_backward_bound(d.qkv, d.dout, d.table, gref, *c.geom, adt)
    runs = []
    for _ in range(2):
        dqkv = _out16(3 * n)
        _run(lib.dmx_htsat_win_attn_bwd_raw(_p(qkv), _p(dout), _p(dqkv), _p(table), B, H, W, c.C, heads, shift, _st()), f"{c} dqkv")
        runs.append(_read16(dqkv, 3 * n, f"{c} dqkv"))
    assert torch.equal(runs[0], runs[1])
    got = _vals16(runs[0]).view(B, H * W, 3, c.C)
    g3, b3 = gref.view(B, H * W, 3, c.C), gb.view(B, H * W, 3, c.C)
    for j, nm in enumerate(("dq", "dk", "dv")):
        _check("win_attn_bwd", f"{c} {nm}", got[:, :, j], g3[:, :, j], b3[:, :, j])


def test_window_attention_refusals():
    lib = _L().lib()
    n = 16 * 16 * 48
    qkv, table = _act(torch.zeros(3 * n, dtype=torch.float64)), _f32(torch.zeros(225 * 2, dtype=torch.float64))
    for (B, H, W, Cc, heads, shift), match in (((1, 12, 16, 48, 2, 0), "multiples of 8"), ((1, 16, 12, 48, 2, 4), "multiples of 8"),
                                               ((1, 16, 16, 40, 2, 0), "x 24"), ((1, 16, 16, 48, 2, 8), "shift"),
                                               ((0, 16, 16, 48, 2, 0), "batch"), ((1, 16, 16, 48, 0, 0), "heads")):
        out, dqkv = _out16(n), _out16(3 * n)
        _refused(lib.dmx_htsat_win_attn_fwd_raw(_p(qkv), _p(out), _p(table), B, H, W, Cc, heads, shift, _st()), "window attention", match)
        _refused(lib.dmx_htsat_win_attn_bwd_raw(_p(qkv), _p(qkv), _p(dqkv), _p(table), B, H, W, Cc, heads, shift, _st()), "window attention backward", match)
        assert bool((out.cpu() == SENT16).all()) and bool((dqkv.cpu() == SENT16).all())


# =============================================================================================================================== embed
_ENGINES = {}


def _engine(E):
    """the input stage alone: a tower without stages (spec_size 64, 32 mel bins: 128 stretched frames, a 16 x 16 token grid)"""
    if E not in _ENGINES:
        from diffmusic_amd.engine import HtsatEngine
        P = N.embed_params(E)
        eng = HtsatEngine(dict(spec_size=N.EMBED_CFG["spec"], num_mel_bins=N.EMBED_CFG["bins"], patch_embeds_hidden_size=E, depths=[],
                               num_attention_heads=[], layer_norm_eps=N.EMBED_CFG["ln_eps"], batch_norm_eps=N.EMBED_CFG["bn_eps"]))
        a = "audio_encoder."
        sd = {a + "batch_norm.weight": P.bn_w, a + "batch_norm.bias": P.bn_b, a + "batch_norm.running_mean": P.bn_m,
              a + "batch_norm.running_var": P.bn_v, a + "patch_embed.proj.weight": P.Wp, a + "patch_embed.proj.bias": P.bp,
              a + "patch_embed.norm.weight": P.ln_g, a + "patch_embed.norm.bias": P.ln_b, a + "norm.weight": torch.ones(E), a + "norm.bias": torch.zeros(E)}
        _ENGINES[E] = eng.load_state_dict(sd, strict=True)
        assert (eng.tokens, eng.channels) == ((N.EMBED_CFG["spec"] // 4) ** 2, E)
    return _ENGINES[E]


@pytest.mark.parametrize("case", N.EMBED_CASES, ids=repr)
def test_embed(case):
    c, adt, lib = case, _adt(), _L().lib()
    d, cfg, eng = c.data(adt), N.embed_config(c.E), _engine(c.E)
    B, frames, bins = d.mel.shape
    Tout, ntok = cfg.spec * (cfg.spec // bins), (cfg.spec // 4) ** 2
    mel, dtok, scale = _f32(d.mel), _act(d.dtok), _f32(d.scale)
    ref = N.embed_forward(d.mel, d.P, cfg)
    n = B * ntok * c.E
    tok = _out16(n)
    _run(lib.dmx_htsat_embed_fwd_raw(eng._h, _p(mel), B, frames, _p(tok), _st()), f"{c} tokens")
    _check("embed_fwd", f"{c} tokens", _vals16(_read16(tok, n, f"{c} tokens")).view(ref.shape), ref, N.embed_forward_bound(d.mel, d.P, cfg, ref, adt))
    dimg_ref, dmel_ref = N.embed_backward(d.mel, d.dtok, d.scale, d.P, cfg)
    b_dimg, b_dmel = N.embed_backward_bound(d.mel, d.dtok, d.scale, d.P, cfg, dimg_ref, dmel_ref)
    runs = []
    for _ in range(2):
        dimg, dmel = _out32(B * Tout * bins), _out32(B * frames * bins)
        _run(lib.dmx_htsat_embed_bwd_raw(eng._h, _p(mel), B, frames, _p(dtok), _p(scale), _p(dimg), _p(dmel), _st()), f"{c} backward")
        runs.append((_read32(dimg, B * Tout * bins, f"{c} dimg"), _read32(dmel, B * frames * bins, f"{c} dmel")))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    _check("embed_bwd", f"{c} dimg", _vals32(runs[0][0]).view(dimg_ref.shape), dimg_ref, b_dimg)
    _check("interp_bwd", f"{c} dmel", _vals32(runs[0][1]).view(dmel_ref.shape), dmel_ref, b_dmel)


def test_embed_refusals():
    lib, eng = _L().lib(), _engine(8)
    mel = _f32(torch.zeros(2 * 129 * 32, dtype=torch.float64))
    dtok = _act(torch.zeros(2 * 256 * 8, dtype=torch.float64))
    for B, frames in ((1, 1), (1, 129), (0, 100)):
        tok, dimg, dmel = _out16(2 * 256 * 8), _out32(2 * 128 * 32), _out32(2 * 129 * 32)
        _refused(lib.dmx_htsat_embed_fwd_raw(eng._h, _p(mel), B, frames, _p(tok), _st()), f"embed frames {frames}", "frames")
        _refused(lib.dmx_htsat_embed_bwd_raw(eng._h, _p(mel), B, frames, _p(dtok), None, _p(dimg), _p(dmel), _st()), f"embed backward frames {frames}", "frames")
        assert bool((tok.cpu() == SENT16).all()) and bool((dimg.cpu() == SENT32).all()) and bool((dmel.cpu() == SENT32).all())
    _refused(lib.dmx_htsat_embed_fwd_raw(None, _p(mel), 1, 100, _p(_out16(8)), _st()), "embed without a handle", "handle")


# ================================================================================================================================ Gram
@pytest.mark.parametrize("case", N.GRAM_CASES, ids=repr)
def test_gram(case):
    c, lib = case, _L().lib()
    d = c.data()
    Fm, dG = _f32(d.F), _f32(d.dG)
    bG, bdF = N.gram_bounds(d.F, d.dG)
    G = _out32(c.B * c.C * c.C)
    _run(lib.dmx_gram_fwd(_p(Fm), _p(G), c.B, c.T, c.C, _st()), f"{c} G")
    ref = N.gram(d.F)
    _check("gram_fwd", f"{c} G", _vals32(_read32(G, c.B * c.C * c.C, f"{c} G")).view(ref.shape), ref, bG)
    runs = []
    for _ in range(2):
        dF = _out32(c.B * c.T * c.C)
        _run(lib.dmx_gram_bwd(_p(Fm), _p(dG), _p(dF), c.B, c.T, c.C, _st()), f"{c} dF")
        runs.append(_read32(dF, c.B * c.T * c.C, f"{c} dF"))
    assert torch.equal(runs[0], runs[1])
    ref = N.gram_backward(d.F, d.dG)
    _check("gram_bwd", f"{c} dF", _vals32(runs[0]).view(ref.shape), ref, bdF)


def test_gram_refusals():
    lib = _L().lib()
    Fm, dG = _f32(torch.zeros(97 * 8, dtype=torch.float64)), _f32(torch.zeros(64, dtype=torch.float64))
    G, dF = _out32(64), _out32(97 * 8)
    _refused(lib.dmx_gram_fwd(_p(Fm), _p(G), 1, N.GRAM_MAX_T + 1, 8, _st()), "gram T 97", "tokens <= 96")
    _refused(lib.dmx_gram_fwd(_p(Fm), _p(G), 1, 0, 8, _st()), "gram T 0", "tokens")
    _refused(lib.dmx_gram_bwd(_p(Fm), _p(dG), _p(dF), 1, 0, 8, _st()), "gram backward T 0", "at least 1")
    _refused(lib.dmx_gram_bwd(_p(Fm), _p(dG), _p(dF), 0, 8, 8, _st()), "gram backward B 0", "at least 1")
    assert bool((G.cpu() == SENT32).all()) and bool((dF.cpu() == SENT32).all())
