"""-m gpu: the tap-stationary ("slab") K loop of the 320 x 256 tile (tile_cfg 20 / 21 / 22, csrc/gemm_tile.h) through dmx_gemm_raw.
Every case is checked two ways: bit for bit against the stock loop of the same tile (tile_cfg 7) on the same buffers -- the K order per
accumulator and the epilogue are the same, so anything but equality is a bug -- and against torch's fp32 convolution within the bound
test_gpu_gemm.py::test_conv1d_dilated uses.  The three clips sit in a larger buffer: the rows before the first and behind the last clip
are NaN, the outer clips are 64 x larger than the middle one, so a halo that bleeds across a clip boundary or a read outside the
clips cannot pass."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, MARGIN, SLOPE = 3, 512, 0.1


def _adt():
    from diffmusic_amd import _lib as L
    return L.act_dtype()


def _desc(L, **kw):
    d = L.GemmDesc()
    d.Z = d.Zi = 1
    d.sy = d.sx = d.osy = d.osx = 1
    d.alpha = 1.0
    for k, v in kw.items():
        if k in ("tdy", "tdx"):
            for i, t in enumerate(v):
                getattr(d, k)[i] = t
        elif isinstance(v, torch.Tensor):
            setattr(d, k, v.data_ptr())
        else:
            setattr(d, k, v)
    return d


def _run(L, d):
    L.check(L.lib().dmx_gemm_raw(C.byref(d), C.sizeof(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "gemm")
    torch.cuda.synchronize()


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _packbits(t):
    b = (t.float() > 0).to(torch.uint8).reshape(*t.shape[:-1], t.shape[-1] // 8, 8)
    w = (2 ** torch.arange(8, device=t.device, dtype=torch.int32)).to(torch.uint8)
    return (b * w).sum(-1).to(torch.uint8).contiguous()


def _slab_cfg(k):
    return 21 if k >= 6 else (20 if k >= 3 else 22)          # slab pieces per wave and K step: 1 / 2 / 3


def _framed(rows, ch, fill):
    """(MARGIN + rows + MARGIN, ch) buffer filled with `fill`; returns it and the view of the `rows` in the middle"""
    big = torch.full((MARGIN + rows + MARGIN, ch), fill, dtype=_adt(), device="cuda")
    return big, big[MARGIN:MARGIN + rows]


def _case(T, Ci, Co, k, dil, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, Ci, generator=g)
    x[0] *= 64.0
    x[2] *= 64.0
    xbig, xv = _framed(B * T, Ci, float("nan"))
    xv.copy_(x.reshape(B * T, Ci).to(_adt()))
    w = (torch.randn(Co, Ci, k, generator=g) / (Ci * k) ** 0.5).to(_adt()).cuda()
    return dict(T=T, Ci=Ci, Co=Co, k=k, dil=dil, pad=(k - 1) * dil // 2, xbig=xbig, x=xv, w=w,
                wp=w.permute(0, 2, 1).reshape(Co, k * Ci).contiguous(), bias=torch.randn(Co, generator=g).cuda(),
                res=torch.randn(B, T, Co, generator=g).to(_adt()).cuda(), act=torch.randn(B, T, Co, generator=g).to(_adt()).cuda())


def _launch(L, c, cfg, mode):
    """one launch of case `c` on tile `cfg`; returns the tensors it wrote (framed outputs included, to see a stray row)"""
    T, Ci, Co, k, dil, pad = c["T"], c["Ci"], c["Co"], c["k"], c["dil"], c["pad"]
    obig, out = _framed(B * T, Co, 7.0)
    out2 = torch.full((B * T, Co), 7.0, dtype=_adt(), device="cuda")
    bits = torch.full((B * T, Co // 8), 0xAA, dtype=torch.uint8, device="cuda")
    fwd = mode in ("fwd", "fwd_bits")
    tdx = [t * dil - pad for t in range(k)] if fwd else [pad - t * dil for t in range(k)]
    kw = dict(A=c["x"], W=c["wp"], C=out, R=c["res"], M=B * T, N=Co, K=k * Ci, ldw=k * Ci, Hi=1, Wi=T, Ci=Ci, lda=Ci, Hq=1, Wq=T, ntaps=k,
              Ho=1, Wo=T, ldc=Co, ldr=Co, ldx=Co, ldc2=Co, tdy=[0] * k, tdx=tdx, tile_cfg=cfg)
    if fwd:
        kw.update(C2=out2, bias=c["bias"], act_slope=SLOPE, flags=L.EPI_BIAS | L.EPI_RESID | L.EPI_LRELU2)
        if mode == "fwd_bits":
            kw.update(B2=bits, ldb2=Co // 8, flags=kw["flags"] | L.EPI_BITS2)
    elif mode == "bwd_mask":
        kw.update(X=c["act"], mask_slope=SLOPE, flags=L.EPI_MASK | L.EPI_RESID)
    else:
        kw.update(XB=_packbits(c["act"]).reshape(B * T, Co // 8), ldxb=Co // 8, mask_slope=SLOPE, flags=L.EPI_MASKBITS | L.EPI_RESID)
    _run(L, _desc(L, **kw))
    assert L.lib().dmx_gemm_last_cfg_raw() == cfg
    return obig, out, out2, bits


def _reference(c, mode):
    xf = c["x"].float().reshape(B, c["T"], c["Ci"]).transpose(1, 2)
    if mode in ("fwd", "fwd_bits"):
        return F.conv1d(xf, c["w"].float(), c["bias"], padding=c["pad"], dilation=c["dil"]).transpose(1, 2) + c["res"].float()
    y = F.conv1d(xf, c["w"].float().flip(-1), None, padding=c["pad"], dilation=c["dil"]).transpose(1, 2)
    return y * torch.where(c["act"].float() > 0, 1.0, SLOPE) + c["res"].float()


def _check(c):
    from diffmusic_amd import _lib as L
    T, Co = c["T"], c["Co"]
    for mode in ("fwd", "fwd_bits", "bwd_mask", "bwd_bits"):
        stock = _launch(L, c, 7, mode)
        slab = _launch(L, c, _slab_cfg(c["k"]), mode)
        for a, b in zip(stock, slab):
            assert torch.equal(a, b), mode                     # (NaN anywhere fails too: NaN != NaN)
        obig, out, out2, bits = slab
        assert float((obig[:MARGIN].float() - 7.0).abs().max()) == 0.0 and float((obig[MARGIN + B * T:].float() - 7.0).abs().max()) == 0.0
        ref = _reference(c, mode)
        assert _rel(out.reshape(B, T, Co), ref) < 6e-3, mode
        # the middle clip alone: its neighbours are 64 x larger and would dominate the norm over all three
        assert _rel(out.reshape(B, T, Co)[1], ref[1]) < 6e-3, mode
        if mode in ("fwd", "fwd_bits"):
            assert _rel(out2.reshape(B, T, Co), F.leaky_relu(ref, SLOPE)) < 6e-3, mode
        if mode == "fwd_bits":
            assert torch.equal(bits, _packbits(out2))


# T: 77 = one partial tile per clip, every slab mostly out of range; 321 = the second tile holds one row; 700 = a clip ends mid-tile
# (a flat tiling of M would straddle clips).  (k, dilation): halos 2 ... 50; k = 11 runs the one-piece-per-step schedule, where the
# next group's slab arrives over 11 steps; k = 3 the two-piece one.
@pytest.mark.parametrize("T", [77, 321, 700])
@pytest.mark.parametrize("k,dil", [(3, 1), (3, 5), (7, 3), (11, 1), (11, 5)])
def test_slab_loop_equals_the_stock_loop(k, dil, T):
    """Ci = 128, Co = 256: two channel groups, one N tile"""
    _check(_case(T, 128, 256, k, dil, seed=100 * k + dil))


def test_four_groups_two_n_tiles():
    """Ci = 256, Co = 512: the slab buffers alternate twice, two N tiles share every slab"""
    _check(_case(700, 256, 512, 7, 3, seed=9))


def test_two_taps_take_three_pieces_per_step():
    """k = 2 (a ConvTranspose phase's dense taps): 6 pieces in 2 steps, the third schedule"""
    from diffmusic_amd import _lib as L
    c = _case(321, 128, 256, 2, 1, seed=11)
    c["pad"] = 0
    T, Ci, Co = c["T"], c["Ci"], c["Co"]
    outs = []
    for cfg in (7, 22):
        out = torch.full((B * T, Co), 7.0, dtype=_adt(), device="cuda")
        _run(L, _desc(L, A=c["x"], W=c["wp"], C=out, M=B * T, N=Co, K=2 * Ci, ldw=2 * Ci, Hi=1, Wi=T, Ci=Ci, lda=Ci, Hq=1, Wq=T, ntaps=2,
                      Ho=1, Wo=T, ldc=Co, ldr=Co, ldx=Co, ldc2=Co, tdy=[0, 0], tdx=[1, 0], tile_cfg=cfg))
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    xf = F.pad(c["x"].float().reshape(B, T, Ci).transpose(1, 2), (0, 1))          # out[q] = W0 x[q + 1] + W1 x[q]
    ref = F.conv1d(xf, c["w"].float().flip(-1), None).transpose(1, 2)
    assert _rel(outs[1].reshape(B, T, Co), ref) < 6e-3


def test_dispatcher_takes_the_slab_loop_for_an_adopted_stage():
    """tile_cfg = 0 at the benchmark's C = 512 stage (8 clips of 5001 frames, k = 3): the dispatcher's own choice is the slab loop, and
    what it computes is what a forced cfg 7 computes"""
    import os
    from diffmusic_amd import _lib as L
    assert not os.environ.get("DMX_NO_SLAB"), "DMX_NO_SLAB is the A/B switch that turns the adopted path off"
    Bq, T, Cc, k = 8, 5001, 512, 3
    g = torch.Generator().manual_seed(13)
    x = torch.randn(Bq * T, Cc, generator=g).to(_adt()).cuda()
    wp = (torch.randn(Cc, k * Cc, generator=g) / (Cc * k) ** 0.5).to(_adt()).cuda()
    bias = torch.randn(Cc, generator=g).cuda()
    outs = []
    for cfg, want in ((0, 20), (7, 7)):
        out = torch.zeros(Bq * T, Cc, dtype=_adt(), device="cuda")
        _run(L, _desc(L, A=x, W=wp, C=out, bias=bias, M=Bq * T, N=Cc, K=k * Cc, ldw=k * Cc, Hi=1, Wi=T, Ci=Cc, lda=Cc, Hq=1, Wq=T, ntaps=k,
                      Ho=1, Wo=T, ldc=Cc, ldr=Cc, ldx=Cc, ldc2=Cc, flags=L.EPI_BIAS, tdy=[0] * k, tdx=[-1, 0, 1], tile_cfg=cfg))
        assert L.lib().dmx_gemm_last_cfg_raw() == want
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


def test_forced_slab_tile_refuses_what_it_cannot_take():
    """a forced tile is an order, not a hint: a launch the slab loop cannot serve is an error, never another kernel"""
    from diffmusic_amd import _lib as L
    c = _case(77, 128, 256, 3, 1, seed=12)
    T, Ci, Co = c["T"], c["Ci"], c["Co"]
    out = torch.zeros(B * T, Co, dtype=_adt(), device="cuda")
    kw = dict(A=c["x"], W=c["wp"], C=out, M=B * T, N=Co, K=3 * Ci, ldw=3 * Ci, Hi=1, Wi=T, Ci=Ci, lda=Ci, Hq=1, Wq=T, ntaps=3,
              Ho=1, Wo=T, ldc=Co, ldr=Co, ldx=Co, ldc2=Co, tdy=[0] * 3, tdx=[-1, 0, 1])
    assert L.lib().dmx_gemm_raw(C.byref(_desc(L, tile_cfg=21, **kw)), C.sizeof(L.GemmDesc), None) != 0      # 3 taps x 1 piece < 6 pieces
    kw["tdx"] = [-40, 0, 40]
    assert L.lib().dmx_gemm_raw(C.byref(_desc(L, tile_cfg=20, **kw)), C.sizeof(L.GemmDesc), None) != 0      # span 80 > 64
    torch.cuda.synchronize()
