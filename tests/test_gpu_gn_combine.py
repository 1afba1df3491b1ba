"""-m gpu: the (group, image) combine of producer-written GroupNorm partial sums -- gn_parts_stats_kernel and gn_bwd_parts_finalize_kernel
(csrc/elementwise.hip), one workgroup per (group, image) -- through the entry points and the producer-GEMM helper of
tests/test_gpu_groupnorm.py.  Every forward case runs twice: statistics only (y = NULL, always the (group, image) kernel) and with the
normalised output (whatever plan dmx_groupnorm_fwd picks for the shape).  References are float64, computed from the fp16 tensor the
producer wrote; bounds are the project's GroupNorm bounds (mean atol 3e-5 / rtol 1e-5, rstd and scale rtol 3e-5, shift atol 3e-5,
y rel-L2 1e-3, dx rel-L2 2e-3 against float64 and 1e-3 against the classic path)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_groupnorm import _conv1x1_with_gnstats

pytestmark = pytest.mark.gpu
EPS = 1e-5


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _produce(L, g, B, P, K, Cc, cfg=0):
    """One producer launch: a 1x1 convolution (+ bias + residual) over B images of P pixels with EPI_GNSTATS.
    Returns (out (B, P, Cc) fp16, partial sums, rows per slot)."""
    x = torch.randn(B * P, K, generator=g).to(L.act_dtype()).cuda()
    w = (torch.randn(Cc, K, generator=g) / K ** 0.5).to(L.act_dtype()).cuda()
    bias = torch.randn(Cc, generator=g).cuda()
    res = (1.5 * torch.randn(B * P, Cc, generator=g) + 0.7).to(L.act_dtype()).cuda()
    out, part, tm = _conv1x1_with_gnstats(L, x, w, bias, res, P, cfg)
    torch.cuda.synchronize()
    assert tm >= 32, f"the producer launch carried no statistics (tm {tm})"
    return out.reshape(B, P, Cc), part, tm


def _affine(g, Cc):
    return (torch.randn(Cc, generator=g) * 0.3 + 1.0).cuda(), (torch.randn(Cc, generator=g) * 0.2).cuda()


def _gn_parts(L, x, gamma, beta, G, silu, regions, with_y):
    """dmx_groupnorm_parts_raw on x (B, P, Cc); regions = [(part, tm, P_region, nq, qoff, cq)].  Returns (y or None, stats, scale, shift)."""
    B, P, Cc = x.shape
    y = torch.empty_like(x) if with_y else None
    stats = torch.full((B, G, 2), float("nan"), device="cuda")
    scale, shift = torch.full((B, Cc), float("nan"), device="cuda"), torch.full((B, Cc), float("nan"), device="cuda")
    geom, ptrs = [], []
    for part, tm, Pr, nq, qoff, cq in regions:
        geom += [tm, Pr, nq, qoff, cq, 0]
        ptrs.append(part.data_ptr())
    n = len(regions)
    L.check(L.lib().dmx_groupnorm_parts_raw(_p(x), _p(y), _p(gamma), _p(beta), _p(stats), _p(scale), _p(shift), B, P, Cc, G, EPS, silu, n,
                                            (C.c_void_p * n)(*ptrs), (C.c_int * (6 * n))(*geom), _stream()), "groupnorm_parts")
    torch.cuda.synchronize()
    return y, stats, scale, shift


def _check_forward(x, gamma, beta, G, silu, regions):
    from diffmusic_amd import _lib as L
    B, P, Cc = x.shape
    cpg = Cc // G
    xd = x.double()
    xg = xd.reshape(B, P, G, cpg)
    mean = xg.mean(dim=(1, 3))
    rstd = (xg.var(dim=(1, 3), unbiased=False) + EPS).rsqrt()
    sc_ref = rstd.repeat_interleave(cpg, dim=1) * gamma.double()
    sh_ref = beta.double() - mean.repeat_interleave(cpg, dim=1) * sc_ref
    ref = F.group_norm(xd.transpose(1, 2), G, gamma.double(), beta.double(), EPS).transpose(1, 2)
    if silu:
        ref = F.silu(ref)
    for with_y in (False, True):
        y, stats, scale, shift = _gn_parts(L, x, gamma, beta, G, silu, regions, with_y)
        e_mean = (stats[..., 0].double() - mean).abs().max().item()
        e_rstd = ((stats[..., 1].double() - rstd).abs() / rstd).max().item()
        e_scale = ((scale.double() - sc_ref).abs() / sc_ref.abs()).max().item()
        e_shift = (shift.double() - sh_ref).abs().max().item()
        print(f"with_y {with_y}: mean abs {e_mean:.2e}  rstd rel {e_rstd:.2e}  scale rel {e_scale:.2e}  shift abs {e_shift:.2e}")
        assert torch.allclose(stats[..., 0].double(), mean, atol=3e-5, rtol=1e-5)
        assert torch.allclose(stats[..., 1].double(), rstd, atol=0, rtol=3e-5)
        assert torch.allclose(scale.double(), sc_ref, atol=0, rtol=3e-5)
        assert torch.allclose(shift.double(), sh_ref, atol=3e-5, rtol=0)
        if with_y:
            r = ((y.double() - ref).norm() / ref.norm()).item()
            print(f"y rel-L2 {r:.2e}")
            assert r < 1e-3


# (B, P, K, Cc, G, silu, cfg, slot rows the case is about or None)
FORWARD = {
    "large_smallest": (3, 8256, 64, 32, 8, 1, 1, 64),      # the large plan (P > 8192) at its smallest: 129 slots of 64 rows
    "large_partial_slot": (3, 8200, 64, 64, 16, 0, 1, 64),  # 128 full slots + one of 8 rows
    "mid": (3, 1000, 64, 32, 8, 1, 0, None),
    "one_group": (3, 1000, 64, 72, 1, 1, 0, None),          # G = 1, C = 8 * 9: 18 quads per slot in the one group
    "many_groups": (3, 1000, 64, 256, 64, 0, 0, None),      # G = 64, 4 channels per group: one quad per slot
}


@pytest.mark.parametrize("name", list(FORWARD))
def test_forward_combine(name):
    from diffmusic_amd import _lib as L
    B, P, K, Cc, G, silu, cfg, want_tm = FORWARD[name]
    g = torch.Generator().manual_seed(1000 + P + Cc)
    x, part, tm = _produce(L, g, B, P, K, Cc, cfg)
    if want_tm:
        assert tm == want_tm, tm
    gamma, beta = _affine(g, Cc)
    _check_forward(x, gamma, beta, G, silu, [(part, tm, P, Cc // 4, 0, Cc // 4)])


def test_forward_combine_four_parity_regions():
    """The layout of an upsample-folded convolution at 8 x 12 -> 16 x 24: four launches over the 96 low-resolution positions of an image,
    one per output parity; output pixel (2 y + py, 2 x + px) comes from launch 2 py + px."""
    from diffmusic_amd import _lib as L
    g = torch.Generator().manual_seed(7)
    B, H, W, K, Cc, G = 3, 8, 12, 64, 64, 8
    q = [_produce(L, g, B, H * W, K, Cc) for _ in range(4)]
    full = torch.empty(B, 2 * H, 2 * W, Cc, dtype=q[0][0].dtype, device="cuda")
    for i in range(4):
        full[:, i // 2::2, i % 2::2] = q[i][0].reshape(B, H, W, Cc)
    gamma, beta = _affine(g, Cc)
    _check_forward(full.reshape(B, 4 * H * W, Cc).contiguous(), gamma, beta, G, 1, [(p, tm, H * W, Cc // 4, 0, Cc // 4) for _, p, tm in q])


def test_forward_combine_concatenation_seam_inside_a_group():
    """Two sources along the channels, 64 + 96 channels in 8 groups of 20: group 3 (channels 60 .. 79) straddles the seam at 64."""
    from diffmusic_amd import _lib as L
    g = torch.Generator().manual_seed(8)
    B, P, K, Ca, Cb, G = 3, 1000, 64, 64, 96, 8
    a, pa, tma = _produce(L, g, B, P, K, Ca)
    b, pb, tmb = _produce(L, g, B, P, K, Cb)
    gamma, beta = _affine(g, Ca + Cb)
    _check_forward(torch.cat([a, b], dim=2).contiguous(), gamma, beta, G, 0,
                   [(pa, tma, P, Ca // 4, 0, Ca // 4), (pb, tmb, P, Cb // 4, Ca // 4, Cb // 4)])


def _forward_and_dgrad(L, g, x, gamma, beta, G, silu, K, cfg):
    """The classic forward for the tape, then dy = a 1x1 dgrad GEMM over the images with EPI_GNBWD.  Returns (dy, part, tm, tape)."""
    B, P, Cc = x.shape
    y = torch.empty_like(x)
    stats, scale, shift = torch.empty(B, G, 2, device="cuda"), torch.empty(B, Cc, device="cuda"), torch.empty(B, Cc, device="cuda")
    partial = torch.empty(L.lib().dmx_groupnorm_scratch_floats(B, Cc, G), device="cuda")
    L.check(L.lib().dmx_groupnorm_raw(_p(x), _p(y), _p(gamma), _p(beta), _p(stats), _p(scale), _p(shift), _p(partial), B, P, Cc, G, EPS, silu,
                                      _stream()), "gn")
    a = torch.randn(B * P, K, generator=g).to(L.act_dtype()).cuda()
    w = (torch.randn(Cc, K, generator=g) / K ** 0.5).to(L.act_dtype()).cuda()
    dy = torch.empty(B * P, Cc, dtype=L.act_dtype(), device="cuda")
    part = torch.full((L.lib().dmx_groupnorm_part_floats(B, P, Cc),), float("nan"), device="cuda")
    d = L.GemmDesc()
    d.Z = d.Zi = 1
    d.sy = d.sx = d.osy = d.osx = 1
    d.alpha = 1.0
    for k, v in dict(A=a, W=w, C=dy, gn_part=part, gnb_x=x, gnb_scale=scale, gnb_shift=shift, gnb_stats=stats).items():
        setattr(d, k, v.data_ptr())
    for k, v in dict(M=B * P, N=Cc, K=K, ldw=K, Hi=1, Wi=P, Ci=K, lda=K, Hq=1, Wq=P, ntaps=1, Ho=1, Wo=P, ldc=Cc, ldr=Cc, ldx=Cc, ldc2=Cc,
                     gnb_ldx=Cc, gnb_silu=silu, gnb_cpg=Cc // G, flags=L.EPI_GNBWD, tile_cfg=cfg).items():
        setattr(d, k, v)
    L.check(L.lib().dmx_gemm_raw(C.byref(d), C.sizeof(d), _stream()), "gemm")
    tm = L.lib().dmx_gemm_last_tile_rows_raw()
    torch.cuda.synchronize()
    assert tm >= 32, f"the dgrad launch carried no statistics (tm {tm})"
    return dy.reshape(B, P, Cc), part, tm, (stats, scale, shift, partial)


def _gn_bwd(L, x, dy, add, tape, G, silu, region):
    """dmx_groupnorm_bwd_raw, from the region's partial sums or (region None) by the classic pass.  Returns (dx, k0, k1)."""
    B, P, Cc = x.shape
    stats, scale, shift, partial = tape
    k0, k1 = torch.full((B, Cc), float("nan"), device="cuda"), torch.full((B, Cc), float("nan"), device="cuda")
    dx = torch.empty_like(x)
    if region is None:
        n, ptrs, geom = 0, None, None
    else:
        part, tm = region
        n, ptrs, geom = 1, (C.c_void_p * 1)(part.data_ptr()), (C.c_int * 6)(tm, P, Cc // 4, 0, Cc // 4, 0)
    L.check(L.lib().dmx_groupnorm_bwd_raw(_p(x), _p(dy), _p(add), _p(dx), _p(stats), _p(scale), _p(shift), _p(k0), _p(k1), _p(partial), B, P, Cc,
                                          G, silu, n, ptrs, geom, _stream()), "gn_bwd")
    torch.cuda.synchronize()
    return dx, k0, k1


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("name", ["large_smallest", "large_partial_slot", "mid"])
def test_backward_finalize(name, silu, with_add):
    from diffmusic_amd import _lib as L
    B, P, K, Cc, G, _, cfg, _ = FORWARD[name]
    g = torch.Generator().manual_seed(2000 + P + Cc + silu)
    x = (torch.randn(B, P, Cc, generator=g) * 1.3 + 2.0 * torch.randn(B, 1, Cc, generator=g)).to(L.act_dtype()).cuda()   # large group means
    gamma, beta = _affine(g, Cc)
    dy, part, tm, tape = _forward_and_dgrad(L, g, x, gamma, beta, G, silu, K, cfg)
    add = torch.randn(B, P, Cc, generator=g).to(L.act_dtype()).cuda() if with_add else None
    dx_parts, _, _ = _gn_bwd(L, x, dy, add, tape, G, silu, (part, tm))
    dx_classic, _, _ = _gn_bwd(L, x, dy, add, tape, G, silu, None)
    xr = x.double().requires_grad_(True)
    yr = F.group_norm(xr.transpose(1, 2), G, gamma.double(), beta.double(), EPS).transpose(1, 2)
    if silu:
        yr = F.silu(yr)
    (gref,) = torch.autograd.grad((yr * dy.double()).sum(), xr)
    if with_add:
        gref = gref + add.double()
    rel = lambda u, v: ((u.double() - v.double()).norm() / v.double().norm()).item()
    r64, rcl, rcl64 = rel(dx_parts, gref), rel(dx_parts, dx_classic), rel(dx_classic, gref)
    print(f"dx rel-L2: parts vs float64 {r64:.2e}  parts vs classic {rcl:.2e}  classic vs float64 {rcl64:.2e}")
    assert r64 < 2e-3
    assert rcl < 1e-3


@pytest.mark.parametrize("name", ["large_smallest", "mid_ragged"])
def test_combine_bits_do_not_depend_on_batch_position_or_size(name):
    """The same image at positions 0, 2 and 4 of B = 5 and alone at B = 1: stats, scale, shift, k0 and k1 are the same bits; so are two
    runs of the same call."""
    from diffmusic_amd import _lib as L
    P, K, Cc, G, silu, cfg = {"large_smallest": (8256, 64, 32, 8, 1, 1), "mid_ragged": (1003, 64, 256, 32, 1, 1)}[name]
    g = torch.Generator().manual_seed(3000 + P)
    order = [0, 1, 0, 2, 0]
    xi, ri = torch.randn(3, P, K, generator=g), 1.5 * torch.randn(3, P, Cc, generator=g) + 0.7
    w = (torch.randn(Cc, K, generator=g) / K ** 0.5).to(L.act_dtype()).cuda()
    bias = torch.randn(Cc, generator=g).cuda()
    gamma, beta = _affine(g, Cc)
    ai = torch.randn(3, P, K, generator=g)
    wb = (torch.randn(Cc, K, generator=g) / K ** 0.5).to(L.act_dtype()).cuda()

    def run(idx):
        B = len(idx)
        x = torch.stack([xi[i] for i in idx]).reshape(B * P, K).to(L.act_dtype()).cuda()
        res = torch.stack([ri[i] for i in idx]).reshape(B * P, Cc).to(L.act_dtype()).cuda()
        out, part, tm = _conv1x1_with_gnstats(L, x, w, bias, res, P, cfg)
        torch.cuda.synchronize()
        assert tm >= 32
        out = out.reshape(B, P, Cc)
        region = [(part, tm, P, Cc // 4, 0, Cc // 4)]
        _, stats, scale, shift = _gn_parts(L, out, gamma, beta, G, silu, region, False)
        again = _gn_parts(L, out, gamma, beta, G, silu, region, False)
        assert torch.equal(stats, again[1]) and torch.equal(scale, again[2]) and torch.equal(shift, again[3])
        # backward: dy from a dgrad launch with EPI_GNBWD on the tape just written
        a = torch.stack([ai[i] for i in idx]).reshape(B * P, K).to(L.act_dtype()).cuda()
        dy = torch.empty(B * P, Cc, dtype=L.act_dtype(), device="cuda")
        bpart = torch.full((L.lib().dmx_groupnorm_part_floats(B, P, Cc),), float("nan"), device="cuda")
        d = L.GemmDesc()
        d.Z = d.Zi = 1
        d.sy = d.sx = d.osy = d.osx = 1
        d.alpha = 1.0
        for k, v in dict(A=a, W=wb, C=dy, gn_part=bpart, gnb_x=out, gnb_scale=scale, gnb_shift=shift, gnb_stats=stats).items():
            setattr(d, k, v.data_ptr())
        for k, v in dict(M=B * P, N=Cc, K=K, ldw=K, Hi=1, Wi=P, Ci=K, lda=K, Hq=1, Wq=P, ntaps=1, Ho=1, Wo=P, ldc=Cc, ldr=Cc, ldx=Cc, ldc2=Cc,
                         gnb_ldx=Cc, gnb_silu=silu, gnb_cpg=Cc // G, flags=L.EPI_GNBWD, tile_cfg=cfg).items():
            setattr(d, k, v)
        L.check(L.lib().dmx_gemm_raw(C.byref(d), C.sizeof(d), _stream()), "gemm")
        btm = L.lib().dmx_gemm_last_tile_rows_raw()
        torch.cuda.synchronize()
        assert btm >= 32
        tape = (stats, scale, shift, None)
        _, k0, k1 = _gn_bwd(L, out, dy.reshape(B, P, Cc), None, tape, G, silu, (bpart, btm))
        _, k0b, k1b = _gn_bwd(L, out, dy.reshape(B, P, Cc), None, tape, G, silu, (bpart, btm))
        assert torch.equal(k0, k0b) and torch.equal(k1, k1b)
        assert bool(torch.isfinite(torch.cat([stats.reshape(B, -1), scale, shift, k0, k1], dim=1)).all())
        return out, stats, scale, shift, k0, k1

    five, one = run(order), run([0])
    assert torch.equal(five[0][0], five[0][2]) and torch.equal(five[0][0], five[0][4]) and torch.equal(five[0][0], one[0][0])   # the producer
    for t5, t1, what in zip(five[1:], one[1:], ("stats", "scale", "shift", "k0", "k1")):
        assert torch.equal(t5[0], t5[2]) and torch.equal(t5[0], t5[4]), f"{what}: differs between batch positions"
        assert not torch.equal(t5[0], t5[1]), f"{what}: another image gave the same bits"
        assert torch.equal(t5[0], t1[0]), f"{what}: B = 5 and B = 1 differ"
