"""Shared by tests/test_gn_bound_host.py (CPU) and tests/test_gpu_gn_elementwise.py (GPU): a float64 model of GroupNorm (+SiLU) forward
and backward as csrc/kernels.h documents it (dmx_groupnorm_fwd / dmx_groupnorm_bwd; forward semantics of torch.nn.GroupNorm), its
element-wise error bound, an fp32 emulation of the documented arithmetic, the case table and mutants of the reference.

The model is written from the documented semantics, not from the kernels.  x: (B, P, C) 16-bit, channels-last; group g holds the
channels [g cpg, (g + 1) cpg), n = P cpg values per (image, group):
    forward    mean = sum x / n,  var = sum (x - mean)^2 / n,  rstd = 1 / sqrt(var + eps)          stats[b, g] = (mean, rstd)
               scale[b, c] = rstd gamma[c],  shift[b, c] = beta[c] - mean scale[b, c],  y = act(x scale + shift),  act = SiLU or identity
    backward   (tape: stats, scale, shift as fp32 INPUTS)  z = x scale + shift,  dz = dy act'(z),  dxh = dz scale
               c1 = sum dxh / n,  c2 = rstd sum dxh (x - mean) / n       (the sums are taken of dxh (x - mean); rstd is applied afterwards)
               k0 = -c1 + c2 rstd mean,  k1 = -c2 rstd,  dx = scale dz + k0 + k1 x (+ add)
    producer   per (image, slot of tm rows, 4-channel quad): (sum v, sum v^2) of the stored values (EPI_GNSTATS) and
               (sum dxh, sum dxh (x - mean)) (EPI_GNBWD); an image's last slot holds its P - (ns - 1) tm remaining rows.

Bound (from the number formats and the shape only, never from a kernel's output).  u32 = 2^-24, eps_a = unit roundoff and tiny =
smallest subnormal of the activation type.  A sum of fp32 terms t_i whose longest chain of additions is d long is off by at most
d u32 sum |t_i| (first order).  d is a closed form per plan -- chunk length per thread, then rows in flight x channels per group, then
the combine -- never the tensor size (P pixels, cpg channels per group, rpb rows in flight, ppb rows per chunk, nchunk chunks, ns slots
of tm rows, qpg quads per group; plans and their geometry: plan() / geom() below, a mirror of the documented thresholds):
    plan                     forward statistics                                   d
    register (two-pass)      4 ceil(P cpg / 1024) + 22                            4 values per unit, 256 threads, a 6 + 16 deep tree
    fused finalize/apply     ceil(ppb / rpb) + min(rpb, ppb) cpg + nchunk         one-pass chunks, combined by one thread per group
    three launches           ceil(ppb / rpb) + min(rpb, ppb) cpg + ceil(nchunk G / 1024) + 22
    backward, classic        as three launches (chunk geometry of the shape, never clamped to 32 chunks)
    producer, fused combine  tm / 2 + 4 + sum over regions (ceil(ns G / 256) + qpg) + ceil(256 / G)
    producer, (g, b) grid    tm / 2 + 4 + sum over regions ceil(ns qpg / 256) + 22
    (a slot: the 64 lanes of a wave own a 64-row x 64-column chunk, tm / 8 rows x 4 channels of a quad each, then 3 shuffle steps)
With sa = sum |x| / n, q = sum x^2 / n:
    d_mean  = (d + 4) u32 sa                                                   (sum, count products, one division)
    d_var   = (d + 6) u32 var + d_mean^2                                        two-pass: sum (x - m')^2 = n var + n (m' - mean)^2
            = (d + 10) u32 q + 2 |mean| d_mean + d_mean^2                        one-pass chunks / slots, Chan-combined in two sweeps
    d_rstd  = max over v' in [max(var - d_var, 0), var + d_var] of |1 / sqrt(v' + eps) - rstd| + 4 u32 rstd        (rsqrt: 2 ulp)
              -- to first order rstd (d_var / (2 (var + eps)) + 4 u32); the interval form stays valid when d_var passes var + eps
              (a constant group at a small eps), because no plan lets a computed variance go below zero
    d_scale = |gamma| d_rstd + 2 u32 |scale|
    d_shift = |scale| d_mean + |mean| d_scale + d_mean d_scale + 2 u32 (|mean scale| + |shift|)
    slack   = 6 u32 (|x scale| + |mean scale| + |beta|)      the fp32 affine in either form: x scale + shift, ((x - mean) rstd) gamma + beta
    (SiLU below z = -87: fp32 exp(-z) overflows, the sigmoid and with it y and dz come out as 0: 2 |ref| joins the bound, < 1e-35 -- twice, so
     that an emulation that loses the value altogether still takes half)
    y       : eps_a |ref| (1 + 1/2 with SiLU: __expf) + tiny / 2 + sup |act'| (|x| d_scale + d_shift + slack),   the sup over z +- that
One-pass: a chunk's M2 is q_k - a_k^2 / n_k and the combine adds n_k (a_k / n_k - mean)^2; an error of a_k moves the two by
(-2 m_k + 2 (m_k - mean)) = -2 mean times it -- hence 2 |mean| d_mean -- and an error of the combined mean cancels to first order
(sum n_k (m_k - mean) = 0).  What remains are the roundings of sum x^2, of a_k m_k and of n_k d^2: at most (d + 10) u32 q.  d_var / var
therefore grows like d u32 E[x^2] / var: that is the documented conditioning of the one-pass plans, which the two-pass register plan
does not have (its d_var is relative to var itself).  The offset families below measure exactly this.
Backward.  e_i = bound of the fp32 error of dxh_i: for SiLU  |dy scale| (0.5 dz_z + (rs + 3 u32) (|silu'| + sig |z|)) + 2 u32 |dxh|
with dz_z = 2 u32 (|x scale| + |shift|), rs = 1.5 (1 - sig) (|z| + 2) u32 + 2 u32 (the relative error of 1 / (1 + __expf(-z)));
without SiLU 2 u32 |dxh|.  k0 and k1 are plain sums of O(1) products:
    d_c1 = (sum e + (d + 2) u32 sum |dxh|) / n
    d_c2 = rstd (sum e |x - mean| + (d + 6) u32 sum |dxh (x - mean)|) / n
    d_k0 = d_c1 + rstd |mean| d_c2 + 3 u32 (|c1| + |c2 rstd mean|),    d_k1 = rstd d_c2 + 2 u32 |k1|
    dx   : eps_a |ref| + tiny / 2 + e + 3 u32 |scale dz| + d_k0 + |x| d_k1 + 3 u32 (|k0| + |k1 x|) + 2 u32 |add| + u32 |ref|
The term 3 u32 (|k0| + |k1 x|) is what remains when |mean| >> std: k0 and k1 x are then large and cancel.
Partial sums of a slot of r rows (4 r values per quad, any order):  4 r u32 sum |v|,  (4 r + 1) u32 sum v^2,  sum e + 4 r u32 sum |dxh|,
sum e |x - mean| + (4 r + 2) u32 sum |dxh (x - mean)|.
Every fp32 product that can underflow adds 2^-149 per term to the bound it enters (gradual underflow; the 16-bit subnormal family, where
a bf16 subnormal times a bf16 subnormal is below the fp32 range altogether).

Sharpness.  Outside the "structure" families (common offsets of 4 and 16 std inside a group: the bound carries E[x^2] / var) the part
of the y and dx bounds that is not the one output rounding exceeds that rounding in at most 10 % of the elements (sharp_fraction();
tests/test_gn_bound_host.py asserts it), so the cases resolve one wrong rounding.  Inputs keep |mean| <= std.  In the chunked passes
one thread adds the min(rpb, ppb) cpg = 2048 / G values a chunk holds of a group; with fewer than 32 groups that chain has 256 .. 2048
links, d u32 reaches eps_a / 30 .. eps_a / 4 in fp16, and outputs within that fraction of the typical magnitude -- more than a tenth of
them when they are spread around zero -- cannot be sharp.  Those shapes keep their outputs away from zero instead: beta = 3 +- 0.2, |dy| >= 1
and add of the sign of dy.  The shapes with G >= 32 (and the subnormal family) carry the outputs around zero.

Emulation share, as in tests/gemm_cases.py: err <= bound / 2 for fp32 outputs; for 16-bit outputs
err <= (eps_a |ref| + tiny / 2) + (bound - eps_a |ref| - tiny / 2) / 2."""
import zlib
from types import SimpleNamespace

import torch

from tests.gemm_cases import U32, SENT16, act_eps, act_tiny

SUP_DSILU = 1.1
EXP_OVER = -87.0                      # fp32 exp(-z) overflows from z = -88.7 on (a fast exp a little earlier): 1 / (1 + exp(-z)) is 0 there
UF32 = 2.0 ** -149                    # an fp32 product that underflows (gradually) is off by at most this
SLACK = 6
GN_SLOT = 64                          # rows per slot of the producers' partial sums (csrc/gemm_epilogue.h)


def cdiv(a, b):
    return -(-a // b)


# --------------------------------------------------------------------------------------------------- plans (documentation only)
def geom(P, C):
    """(threads, rows in flight, chunks, rows per chunk) of the chunked passes"""
    cpr = C >> 3
    rpb = 1 if cpr >= 256 else 256 // cpr
    nchunk = max(1, min(512, cdiv(P, rpb * 8)))
    ppb = cdiv(P, nchunk)
    return cpr * rpb, rpb, cdiv(P, ppb), ppb


def plan(P, C, G, with_y):
    """-> (plan name, rpb, nchunk, ppb) of the classic forward entry"""
    cpg = C // G
    small_fits = cpg % 4 == 0 and cpg <= 256 and P * (cpg // 4) <= 4096
    mid = with_y and 512 <= P <= 8192 and (C >> 3) <= 256
    nt, rpb, nchunk, ppb = geom(P, C)
    if small_fits and not mid:
        return "register", rpb, nchunk, ppb
    if mid:
        cmax = 32
        while cmax > 1 and cmax * G > 8 * max(nt, 64):
            cmax -= 1
        if nchunk > cmax:
            ppb = cdiv(P, cmax)
            nchunk = cdiv(P, ppb)
        return "fused", rpb, nchunk, ppb
    return "three", rpb, nchunk, ppb


def parts_plan(P, C, with_y, regions):
    """regions: [(tm, P_region, nq)] -> plan name of the producer entry"""
    f2 = sum((Pr // tm + 2) * nq for tm, Pr, nq in regions)
    return "parts_fused" if with_y and P <= 8192 and (C >> 3) <= 256 and f2 * 8 < 32 * 1024 else "parts_stats"


def adds(name, P, C, G, rpb=0, nchunk=0, ppb=0, regions=()):
    """longest chain of additions of a plan's statistics (module docstring).  regions: [(tm, slots, quads of a group)]"""
    cpg = C // G
    if name == "register":
        return 4 * cdiv(P * cpg, 1024) + 22
    if name == "fused":
        return cdiv(ppb, rpb) + min(rpb, ppb) * cpg + nchunk
    if name == "three":
        return cdiv(ppb, rpb) + min(rpb, ppb) * cpg + cdiv(nchunk * G, 1024) + 22
    tm = max(r[0] for r in regions)
    if name == "parts_fused":
        return tm // 2 + 4 + sum(cdiv(ns * G, 256) + qpg for _, ns, qpg in regions) + cdiv(256, G)
    assert name == "parts_stats", name
    return tm // 2 + 4 + sum(cdiv(ns * qpg, 256) for _, ns, qpg in regions) + 22


def bwd_adds(P, C, G):
    _, rpb, nchunk, ppb = geom(P, C)
    return adds("three", P, C, G, rpb, nchunk, ppb)


def tails(P, rpb, nchunk, ppb):
    """-> (set of the row counts a thread of the LAST chunk has left after its 4-deep loop, last chunk shorter than rpb)"""
    last = P - (nchunk - 1) * ppb
    left = {cdiv(last - r, rpb) % 4 for r in range(min(rpb, last))}
    return left, last < rpb


# ------------------------------------------------------------------------------------------------------------------ the model
def _groups(C, G, mut=None):
    cpg = C // G
    c = torch.arange(C)
    gid = ((c + 1) // cpg).clamp(max=G - 1) if mut == "group_boundary" else c // cpg
    return gid, torch.nn.functional.one_hot(gid, G).double()


def _silu(z):
    return z * torch.sigmoid(z)


def _dsilu(z):
    s = torch.sigmoid(z)
    return s * (1.0 + z * (1.0 - s))


def _sup_dsilu(lo, hi):
    """sup |silu'| over [lo, hi]: silu'' changes sign only at +-2.3994 (silu' = 1.0998 and -0.0998 there), so the sup sits at an end or there"""
    s = torch.maximum(_dsilu(lo).abs(), _dsilu(hi).abs())
    for c, v in ((-2.3994, 0.0999), (2.3994, SUP_DSILU)):
        s = torch.where((lo < c) & (hi > c), s.clamp_min(v), s)
    return s


def forward(x, gamma, beta, G, eps, silu, mut=None, with_y=True):
    """x (B, P, C) float64 (the 16-bit values), gamma / beta (C) float64 -> namespace mean, rstd, var, q, sa (B, G); scale, shift (B, C); y"""
    B, P, C = x.shape
    gid, M = _groups(C, G, mut)
    if mut == "affine_shift":
        gamma, beta = gamma.roll(1), beta.roll(1)
    rows = cdiv(P, GN_SLOT) * GN_SLOT if mut == "last_slot_full" else P
    cnt = M.sum(0) * rows
    s1 = x.sum(1)
    mean = (s1 @ M) / cnt
    q = ((x * x).sum(1) @ M) / cnt
    sa = (x.abs().sum(1) @ M) / cnt
    var = (q - mean * mean).clamp_min(0.0)
    if mut == "unbiased":
        var = var * cnt / (cnt - 1)
    rstd = 1.0 / torch.sqrt(var + (0.0 if mut == "no_eps" else eps))
    scale = rstd[:, gid] * gamma
    mean_c = s1 / P if mut == "mean_per_channel" else mean[:, gid]
    shift = beta - mean_c * scale
    r = SimpleNamespace(mean=mean, rstd=rstd, var=var, q=q, sa=sa, scale=scale, shift=shift, y=None)
    if with_y:
        sc, sh = (scale.roll(-1, 0), shift.roll(-1, 0)) if mut == "next_image" else (scale, shift)
        z = x * sc[:, None] + sh[:, None]
        r.y = _silu(z) if silu else z
    return r


def forward_bound(x, gamma, beta, G, eps, silu, r, d, two_pass, adt, with_y=True):
    """element-wise bounds of forward()'s outputs for a plan with chain length d -> namespace mean, rstd, scale, shift, y, y_round"""
    gid, _ = _groups(x.shape[2], G)
    d_mean = (d + 4) * U32 * r.sa
    if two_pass:
        d_var = (d + 6) * U32 * r.var + d_mean * d_mean + 2 * UF32
    else:
        d_var = (d + 10) * U32 * r.q + 2 * r.mean.abs() * d_mean + d_mean * d_mean + 2 * UF32
    lo = 1.0 / torch.sqrt(r.var + d_var + eps)
    hi = 1.0 / torch.sqrt((r.var - d_var).clamp_min(0.0) + eps)
    d_rstd = torch.maximum(r.rstd - lo, hi - r.rstd) + 4 * U32 * r.rstd
    d_scale = gamma.abs() * d_rstd[:, gid] + 2 * U32 * r.scale.abs()
    mc, dm = r.mean[:, gid], d_mean[:, gid]
    d_shift = r.scale.abs() * dm + mc.abs() * d_scale + dm * d_scale + 2 * U32 * ((mc * r.scale).abs() + r.shift.abs()) + UF32
    b = SimpleNamespace(mean=d_mean, rstd=d_rstd, scale=d_scale, shift=d_shift, y=None, y_round=None)
    if with_y:
        ea, tiny = act_eps(adt), act_tiny(adt)
        slack = SLACK * U32 * ((x * r.scale[:, None]).abs() + ((mc * r.scale).abs() + beta.abs())[:, None])
        carried = x.abs() * d_scale[:, None] + d_shift[:, None] + slack + 2 * UF32
        b.y_round = ea * r.y.abs() + tiny / 2
        if silu:
            z = x * r.scale[:, None] + r.shift[:, None]
            gone = torch.where(z - carried < EXP_OVER, 2 * r.y.abs(), torch.zeros((), dtype=torch.float64))
            carried = 0.5 * ea * r.y.abs() + _sup_dsilu(z - carried, z + carried) * carried + gone
        b.y = b.y_round + carried
    return b


def tape_bound(x, y_ref, scale, shift, mean_scale_beta, silu, adt):
    """bound of y against act(x scale_k + shift_k) taken in float64 from the tape a kernel wrote itself: the output rounding and the fp32
    slack of the affine, nothing carried from the statistics.  mean_scale_beta: (B, C) |mean scale| + |beta|"""
    ea, tiny = act_eps(adt), act_tiny(adt)
    slack = SLACK * U32 * ((x * scale[:, None]).abs() + mean_scale_beta[:, None]) + 2 * UF32
    return ea * y_ref.abs() * (1.5 if silu else 1.0) + tiny / 2 + (SUP_DSILU if silu else 1.0) * slack


def backward(x, dy, add, mean, rstd, scale, shift, G, silu, mut=None):
    """closed-form backward from a given tape (float64 values of fp32 inputs) -> namespace k0, k1 (B, C), dx, and what the bound needs"""
    B, P, C = x.shape
    gid, M = _groups(C, G, mut)
    n = P * (C // G)
    if mut == "next_image":
        scale, shift = scale.roll(-1, 0), shift.roll(-1, 0)
    sc = scale[:, None]
    z = x * sc + shift[:, None]
    if silu:
        dact = torch.sigmoid(z) if mut == "silu_sigmoid" else _dsilu(z)
        dz = dy * dact
    else:
        dz = dy
    dxh = dz * sc
    xm = x - mean[:, gid][:, None]
    t1, t2 = dxh.sum(1) @ M, (dxh * xm).sum(1) @ M
    c1, c2 = t1 / n, rstd * t2 / n
    k0 = (-c1 + c2 * rstd * mean)[:, gid]
    k1 = (-c2 * rstd)[:, gid]
    if mut == "k1_sign":
        k1 = -k1
    dx = sc * dz + k0[:, None] + k1[:, None] * x
    if add is not None and mut != "drop_add":
        dx = dx + add
    return SimpleNamespace(k0=k0, k1=k1, dx=dx, z=z, dz=dz, dxh=dxh, xm=xm, c1=c1, c2=c2)


def dxh_err(x, dy, scale, shift, r, silu):
    """e: bound of the fp32 error of every dxh (module docstring)"""
    if not silu:
        return 2 * U32 * r.dxh.abs() + 2 * UF32
    sc = scale[:, None]
    sg = torch.sigmoid(r.z)
    dz_z = 2 * U32 * ((x * sc).abs() + shift.abs()[:, None])
    rs = 1.5 * (1.0 - sg) * (r.z.abs() + 2.0) * U32 + 2 * U32
    rs = torch.where(r.z - dz_z < EXP_OVER, torch.full((), 2.0, dtype=torch.float64), rs)          # the sigmoid may come out as 0
    return (dy * sc).abs() * (0.5 * dz_z + (rs + 3 * U32) * (_dsilu(r.z).abs() + sg * r.z.abs())) + 2 * U32 * r.dxh.abs() + 2 * UF32


def backward_bound(x, dy, add, mean, rstd, scale, shift, G, silu, r, d, adt):
    """-> namespace k0, k1 (B, C), dx, dx_round"""
    B, P, C = x.shape
    gid, M = _groups(C, G)
    n = P * (C // G)
    e = dxh_err(x, dy, scale, shift, r, silu)
    d_c1 = (e.sum(1) @ M + (d + 2) * U32 * (r.dxh.abs().sum(1) @ M)) / n
    d_c2 = rstd * ((e * r.xm.abs()).sum(1) @ M + (d + 6) * U32 * ((r.dxh * r.xm).abs().sum(1) @ M)) / n + 2 * UF32 * rstd
    d_k0 = d_c1 + rstd * mean.abs() * d_c2 + 3 * U32 * (r.c1.abs() + (r.c2 * rstd * mean).abs()) + 2 * UF32
    d_k1 = rstd * d_c2 + 2 * U32 * (r.c2 * rstd).abs() + UF32
    d_k0, d_k1 = d_k0[:, gid], d_k1[:, gid]
    ea, tiny = act_eps(adt), act_tiny(adt)
    dx_round = ea * r.dx.abs() + tiny / 2
    carried = e + 3 * U32 * (scale[:, None] * r.dz).abs() + d_k0[:, None] + x.abs() * d_k1[:, None] \
        + 3 * U32 * (r.k0[:, None].abs() + (r.k1[:, None] * x).abs()) + U32 * r.dx.abs() + 4 * UF32
    if add is not None:
        carried = carried + 2 * U32 * add.abs()
    return SimpleNamespace(k0=d_k0, k1=d_k1, dx=dx_round + carried, dx_round=dx_round)


def slot_sum(v, tm):
    """(B, P, C) -> (B, slots, C / 4): sums over the rows of a slot and the 4 channels of a quad; the last slot is the remaining rows"""
    B, P, C = v.shape
    ns = cdiv(P, tm)
    pad = torch.zeros(B, ns * tm, C, dtype=v.dtype)
    pad[:, :P] = v
    return pad.view(B, ns, tm, C // 4, 4).sum(dim=(2, 4))


def slot_rows(P, tm, mut=None):
    ns = cdiv(P, tm)
    rows = torch.full((ns,), float(tm), dtype=torch.float64)
    if mut != "last_slot_full":
        rows[-1] = P - (ns - 1) * tm
    return rows


def forward_slots(v, tm):
    """-> (sum v, sum v^2) per (image, slot, quad) and their bounds"""
    r4 = 4 * slot_rows(v.shape[1], tm)[None, :, None]
    s, q = slot_sum(v, tm), slot_sum(v * v, tm)
    return (s, r4 * U32 * slot_sum(v.abs(), tm)), (q, (r4 + 1) * U32 * q + r4 * UF32)


def backward_slots(x, dy, scale, shift, r, silu, tm):
    """-> (sum dxh, sum dxh (x - mean)) per (image, slot, quad) and their bounds; r = backward() of the same tape"""
    r4 = 4 * slot_rows(x.shape[1], tm)[None, :, None]
    e = dxh_err(x, dy, scale, shift, r, silu)
    t = r.dxh * r.xm
    return ((slot_sum(r.dxh, tm), slot_sum(e, tm) + r4 * U32 * slot_sum(r.dxh.abs(), tm)),
            (slot_sum(t, tm), slot_sum(e * r.xm.abs(), tm) + (r4 + 2) * U32 * slot_sum(t.abs(), tm) + r4 * UF32))


def sharp_fraction(bound, rounding):
    """fraction of the elements whose bound exceeds twice the one output rounding"""
    return ((bound - rounding) > rounding).double().mean().item()


def emu_limit(bound, rounding=None):
    """what the emulation has to stay inside (module docstring)"""
    return bound / 2 if rounding is None else rounding + (bound - rounding) / 2


# ------------------------------------------------------------------------------------------------------------- fp32 emulation
def _f(t):
    return t.float()


def _chunk_sums(v, rows_per, G):
    """(B, P, C) fp32 -> fp32 sums over the rows of a chunk and the channels of a group (B, chunks, G), and the rows of each chunk"""
    B, P, C = v.shape
    nk = cdiv(P, rows_per)
    pad = torch.zeros(B, nk * rows_per, C, dtype=torch.float32)
    pad[:, :P] = v
    s = pad.view(B, nk, rows_per, G, C // G).sum(dim=(2, 4), dtype=torch.float32)
    rows = torch.full((nk,), float(rows_per), dtype=torch.float32)
    rows[-1] = P - (nk - 1) * rows_per
    return s, rows


def _chan(a, qq, nb, eps):
    """items (B, K, G) of (sum, sum of squares, count (K) or (K, G)) -> (mean, rstd) fp32: one-pass M2 per item, Chan-combined in two sweeps"""
    nb = nb.view(1, -1, 1) if nb.dim() == 1 else nb[None]
    m = a / nb
    m2 = (qq - a * m).clamp_min(0.0)
    sn = nb.sum(1, dtype=torch.float32)
    mean = (nb * m).sum(1, dtype=torch.float32) / sn
    dd = m - mean[:, None]
    tot = (m2 + nb * dd * dd).sum(1, dtype=torch.float32)
    return mean, torch.rsqrt(tot / sn + torch.tensor(eps, dtype=torch.float32))


def emulate_forward(x, gamma, beta, G, eps, silu, adt, name, ppb=0, regions=None, with_y=True):
    """fp32 arithmetic as documented -> namespace mean, rstd, scale, shift (float64 values of fp32), y (float64 values of adt).
    name: 'register' (two-pass), 'fused' / 'three' (one-pass chunks of ppb rows), 'parts_*' (one-pass (slot, quad) items;
    regions: [(tm, first channel, channels)], the sources of a concatenation along the channels)"""
    B, P, C = x.shape
    cpg = C // G
    xf, gf, bf = _f(x), _f(gamma), _f(beta)
    gid = torch.arange(C) // cpg
    if name == "register":
        n = torch.tensor(float(P * cpg), dtype=torch.float32)
        xg = xf.view(B, P, G, cpg)
        mean = xg.sum(dim=(1, 3), dtype=torch.float32) / n
        dd = xg - mean[:, None, :, None]
        rstd = torch.rsqrt((dd * dd).sum(dim=(1, 3), dtype=torch.float32) / n + torch.tensor(eps, dtype=torch.float32))
    elif name in ("fused", "three"):
        a, rows = _chunk_sums(xf, ppb, G)
        qq, _ = _chunk_sums(xf * xf, ppb, G)
        mean, rstd = _chan(a, qq, rows * cpg, eps)
    else:
        items = [([], [], []) for _ in range(G)]                  # per group: the (slot, quad) items of every region
        for tm, c0, cn in regions:
            sl = xf[:, :, c0:c0 + cn]
            a, rows = _chunk_sums(sl, tm, cn // 4)                 # (B, slots, quads of the source)
            qq, _ = _chunk_sums(sl * sl, tm, cn // 4)
            for qi in range(cn // 4):
                ia, iq, inb = items[(c0 + 4 * qi) // cpg]
                ia.append(a[:, :, qi]); iq.append(qq[:, :, qi]); inb.append(4 * rows)
        per = [_chan(torch.cat(ia, 1)[:, :, None], torch.cat(iq, 1)[:, :, None], torch.cat(inb), eps) for ia, iq, inb in items]
        mean, rstd = torch.cat([m for m, _ in per], 1), torch.cat([r for _, r in per], 1)
    scale = rstd[:, gid] * gf
    shift = bf - mean[:, gid] * scale
    out = SimpleNamespace(mean=mean.double(), rstd=rstd.double(), scale=scale.double(), shift=shift.double(), y=None)
    if with_y:
        if name == "register":
            z = (xf - mean[:, gid][:, None]) * rstd[:, gid][:, None] * gf + bf
        else:
            z = xf * scale[:, None] + shift[:, None]
        if silu:
            z = z / (1.0 + torch.exp(-z))
        out.y = z.to(adt).double()
    return out


def emulate_backward(x, dy, add, mean, rstd, scale, shift, G, silu, adt, rows_per):
    """fp32: chunk (or slot) sums of dxh and dxh (x - mean), rstd applied afterwards, plain sums of the chunks, k0 / k1, dx stored as adt"""
    B, P, C = x.shape
    cpg = C // G
    gid = torch.arange(C) // cpg
    xf, df, mu, rs, sc, sf = _f(x), _f(dy), _f(mean), _f(rstd), _f(scale)[:, None], _f(shift)[:, None]
    z = xf * sc + sf
    if silu:
        s = 1.0 / (1.0 + torch.exp(-z))
        dz = df * (s * (1.0 + z * (1.0 - s)))
    else:
        dz = df
    dxh = dz * sc
    a, _ = _chunk_sums(dxh, rows_per, G)
    qq, _ = _chunk_sums(dxh * (xf - mu[:, gid][:, None]), rows_per, G)
    n = torch.tensor(float(P * cpg), dtype=torch.float32)
    t1, t2 = a.sum(1, dtype=torch.float32), (qq * rs[:, None]).sum(1, dtype=torch.float32)
    c1, c2 = t1 / n, t2 / n
    k0, k1 = (-c1 + c2 * rs * mu)[:, gid], (-c2 * rs)[:, gid]
    v = sc * dz + k0[:, None] + k1[:, None] * xf
    if add is not None:
        v = v + _f(add)
    return SimpleNamespace(k0=k0.double(), k1=k1.double(), dx=v.to(adt).double())


# ------------------------------------------------------------------------------------------------------------------ the cases
class Case:
    """One forward shape with its data family.  bwd: the (silu, add) variants of the classic backward on the same x."""

    def __init__(self, name, P, C, G, B=3, with_y=True, silu=1, eps=1e-5, family="plain"):
        self.name, self.P, self.C, self.G, self.B, self.with_y, self.silu, self.eps, self.family = name, P, C, G, B, with_y, silu, eps, family
        self.structure = family in ("off4", "off16")
        self.plan, self.rpb, self.nchunk, self.ppb = plan(P, C, G, with_y)
        self.d = adds(self.plan, P, C, G, self.rpb, self.nchunk, self.ppb)
        self.two_pass = self.plan == "register"
        self.away = G < 32                               # a thread of the chunked passes adds 2048 / G values of a group (module docstring)
        self.bwd = [(0, False), (0, True), (1, False), (1, True)]
        self.bwd_d, self.bwd_ppb = bwd_adds(P, C, G), geom(P, C)[3]

    def __repr__(self):
        return self.name

    def data(self, adt):
        """-> namespace x, dy, add (B, P, C) float64 values of adt; gamma, beta (C) float64 values of fp32"""
        g = torch.Generator().manual_seed(zlib.crc32(self.name.encode()))
        B, P, C, G = self.B, self.P, self.C, self.G
        cpg = C // G
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        fam = self.family
        gamma = 1.0 + 0.3 * rn(C)
        beta = 0.2 * rn(C)
        dy = rn(B, P, C)
        if self.away:
            beta = 3.0 + 0.2 * rn(C)
            dy = torch.sign(dy) * (1.0 + 0.25 * dy.abs())
        x = 0.6 + 1.7 * rn(B, P, C)
        xg = x.view(B, P, G, cpg)
        g1, g2 = 1 % G, 2 % G
        if fam == "const":
            xg[0, :, g1] = 0.0
            xg[1, :, g2] = 3.0
        elif fam == "near":
            ulp = 2.0 * torch.finfo(adt).eps                                    # spacing of adt in [2, 4)
            xg[0, :, g1] = 3.0 + ulp * (torch.rand(P, cpg, generator=g, dtype=torch.float64) < 0.5).double()
        elif fam in ("off4", "off16"):
            off = 4.0 if fam == "off4" else 16.0
            sign = torch.where(torch.arange(G) % 2 == 0, 1.0, -1.0).double()
            x = (rn(B, P, G, cpg) + (off * sign)[None, None, :, None]).view(B, P, C)
        elif fam == "gamma30":
            big = (torch.arange(C) // cpg) % 8 == 1                            # every channel of groups 1, 9, ...: |z| passes 89 at 3 std
            gamma = torch.where(big, 30.0 * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).double() * (1.0 + 0.05 * rn(C)), gamma)
        elif fam == "subn":
            s = torch.finfo(adt).smallest_normal / 4
            x = s * rn(B, P, C)
            dy = s * rn(B, P, C)
        else:
            assert fam == "plain", fam
        rd = lambda t: t.to(adt).double()
        add = rn(B, P, C)
        if self.away:
            add = torch.sign(dy) * add.abs()
        return SimpleNamespace(x=rd(x.reshape(B, P, C)), dy=rd(dy), add=rd(add), gamma=gamma.float().double(), beta=beta.float().double())


def _table():
    cs = []
    add = lambda *a, **k: cs.append(Case(*a, **k))
    # register plan
    add("reg-p1", 1, 32, 8)
    add("reg-unet", 64, 640, 32)
    add("reg-cpg256", 16, 1024, 4, silu=0)
    add("reg-4096units", 256, 512, 8)
    add("reg-g64", 252, 256, 64)
    add("reg-g1", 500, 8, 1, silu=0)
    add("reg-stats-only", 1000, 32, 8, with_y=False)
    # three launches below 512 pixels
    add("three-cpg1", 40, 32, 32)
    add("three-cpg2", 160, 64, 32, silu=0)
    add("three-cpg3", 100, 24, 8)
    add("three-p4", 4, 8, 4)
    add("three-4097units", 257, 512, 8)
    add("reg-p511", 511, 128, 32)                 # 4 channels per group: 511 units, the register plan up to the last pixel count below 512
    add("three-p511", 511, 64, 32)                # the same threshold with 2 channels per group
    # fused finalize / apply
    add("fused-p512", 512, 128, 32)
    add("fused-g1", 512, 8, 1, silu=0)
    add("fused-ragged", 1003, 640, 32)
    add("fused-30chunks", 4000, 384, 64, silu=0)
    add("fused-32x64", 8192, 64, 64)
    add("fused-c2048", 1000, 2048, 32, B=2)
    # three launches above 8192 pixels
    add("three-p8193", 8193, 64, 64)
    add("three-512chunks", 8704, 1024, 64, B=1)
    add("three-g2-stats-only", 8200, 128, 2, with_y=False)
    # ragged tails: last chunk leaves 1 / 2 / 3 rows per thread after the 4-deep loop, or is shorter than the rows in flight
    for nm, P, C, G in RAGGED:
        add(nm, P, C, G)
    # data families, one shape per plan
    for pl, (P, C, G) in FAMILY_SHAPES.items():
        add(f"{pl}-const-eps5", P, C, G, family="const")
        add(f"{pl}-const-eps6", P, C, G, family="const", eps=1e-6, silu=0)
        add(f"{pl}-near", P, C, G, family="near")
        add(f"{pl}-off4", P, C, G, family="off4")
        add(f"{pl}-off16", P, C, G, family="off16", silu=0)
        add(f"{pl}-gamma30", P, C, G, family="gamma30")
        add(f"{pl}-subn", P, C, G, family="subn")
    return cs


FAMILY_SHAPES = {"register": (64, 128, 8), "three": (300, 64, 32), "fused": (520, 64, 8)}
# (name, P, C, G): found with tails(); tests/test_gn_bound_host.py asserts what each is there for
RAGGED = [("fused-tail1", 1489, 256, 32), ("fused-tail2", 576, 64, 8), ("fused-tail3", 672, 64, 8), ("fused-short", 530, 640, 32),
          ("three-tail1", 320, 64, 32), ("three-tail2", 384, 64, 32), ("three-tail3", 448, 64, 32)]      # (three-cpg1 and three-p4: one chunk, shorter than the rows in flight)
CASES = _table()
ROUND_TRIP = ["reg-unet", "three-p511", "fused-p512", "three-p8193"]             # backward additionally from the tape the forward kernel wrote

# producer route: (name, tile config, B, P, K, C, G, silu): one tile configuration per statistics tile family (256 x 256, 256 x 128,
# 512 x 128, 128 x 128 LDS-DMA, register-staged 128 x 128), images of 1003 / 700 / 64 / 8256 rows, 8 / 20 / 4 channels per group
PRODUCER = [("prod-256x256", 1, 3, 1003, 64, 256, 32, 1), ("prod-256x128", 2, 3, 700, 64, 640, 32, 0), ("prod-512x128", 19, 3, 64, 64, 128, 32, 1),
            ("prod-128x128-large", 11, 3, 8256, 64, 32, 8, 1), ("prod-regstaged", 3, 3, 1003, 64, 128, 32, 0)]

FWD_MUTANTS = ["unbiased", "no_eps", "group_boundary", "affine_shift", "next_image", "mean_per_channel", "last_slot_full"]
BWD_MUTANTS = ["silu_sigmoid", "drop_add", "k1_sign", "group_boundary", "next_image"]
