"""Shared by tests/test_gemm_bound_host.py (CPU) and tests/test_gpu_gemm_elementwise.py (GPU): a float64 model of the implicit-GEMM
descriptor (csrc/dmx_common.h GemmDesc), its element-wise error bound, an fp32 emulation of the kernels' arithmetic, descriptor
builders for the operations the models run, the case table and mutants of the reference.

The model is written from the documented semantics of GemmDesc, not from the kernels.  Every buffer is a FLAT array that the
descriptor addresses with its own strides (lda / ldw / ldc / ldr / ldx / ldc2 / ldrb, the Z strides, the row maps), so that a wrong
stride, a wrong row map or a store outside the writable set shows up as a wrong element:
    input pixel   iy = qy * sy + tdy[t],  ix = qx * sx + tdx[t]   (zero outside [0, Hi) x [0, Wi))
    output pixel  oy = qy * osy + ooy,    ox = qx * osx + oox
    epilogue      (LN fold) -> mask | softbwd -> bias -> rowbias -> GEGLU -> residual (RESID_INV) -> alpha -> accum -> tanh -> C,
                  then LRELU2 -> C2

Bound (from the number formats only, never from a kernel's output).  u32 = 2^-24, eps = unit roundoff and tiny = smallest subnormal
of the output type.  S = sum_k |a| |w| plus the magnitude of every fp32 addend (bias, row bias, residual, previous C), carried through
the pointwise chain like the value itself (mask factor <= 1, |alpha|):
    accumulation term   A = 2 (K + E) u32 S          E = number of fp32 epilogue operations
    output term         1.5 eps |ref| + tiny / 2     (16-bit; the extra half eps covers the fp32 erfc / tanh)
                        4 u32 |ref|                  (fp32)
    |out - ref| <= A' + output term,  A' = A carried through tanh (slope <= 1), leaky-relu (slope <= 1) and, for GEGLU,
                   |gelu(g)| A_v + |v| sup|gelu'| A_g + A_v A_g sup|gelu'|   with the sup over g +- A_g.
The factor 2 covers an MFMA whose internal adds do not round to nearest (nobody has measured that here; the GPU tests print the
observed err / bound per case).  K <= 72 cases are sharp: A exceeds the output term in at most 10 % of their elements
(sharp_fraction(); tests/test_gemm_bound_host.py asserts it), so that they resolve one wrong rounding of the output.  The deep-K cases
(forced split-K plans, K = 576) are there for structure -- slices, the reduce kernel's epilogue -- and their bound is about twice
one output rounding in the median (fp16: 1.9).

EPI_LNFOLD: v = rstd (acc - mean colsum) + b'.  The reference takes mean / rstd from the exact row sums of the 16-bit rows; the
kernel takes them from fp32 slot sums (sum x, sum x^2 per slot, each rounded once by its producer) added in fp32, and the variance as
E[x^2] - mean^2.  With ns slots, sa = sum |x|, q = sum x^2:
    d_mean <= (ns + 2) u32 sa / K
    d_var  <= (ns + 3) u32 q / K + 2 |mean| d_mean + 3 u32 mean^2
    d_rstd <= rstd (d_var / (2 (var + ln_eps)) + 4 u32)                      (rsqrt: 2 ulp)
    d_t    <= A_acc + |colsum| d_mean + 3 u32 |mean colsum| + u32 |t|        t = acc - mean colsum, colsum rounded to fp32 once
    d_v    <= rstd d_t + |t| d_rstd + 2 u32 (|rstd t| + |b'|)
Rows keep |mean| <= std (the large-offset rows stay with the norm test in tests/test_gpu_gemm.py): then every term above is of the
order of K u32 |v| and the bound stays at rounding level.  The fp32 emulation below validates it.

Sign-bit tape (the two flags the vocoder's tape uses).  EPI_MASKBITS is EPI_MASK with the factor taken from a bit of XB (Buf kind 'bits':
one byte per 8 channels, bit e of byte k <=> channel 8 k + e > 0).  EPI_BITS2 is a third kind of write, compared EXACTLY: when the 16-bit
tensor is stored next to it (C2, or C without EPI_LRELU2) every byte must equal the sign bits of what the kernel itself stored, element for
element; when nothing is stored (the fused pair's bits-only tape, tests/pair_cases.py) it must equal (ref > 0) wherever |ref| > A + tiny and
is free elsewhere.  Untouched bytes keep the sentinel 0xAA.

Emulation share: one rounding to a 16-bit output alone costs up to eps |ref| + tiny / 2, i.e. 2 / 3 of the output term 1.5 eps |ref|, so
"half the bound" cannot hold for the whole error of a 16-bit output.  The host test therefore asserts half for everything EXCEPT that
single rounding: err <= (eps |ref| + tiny / 2) + (bound - eps |ref| - tiny / 2) / 2; for fp32 outputs plainly err <= bound / 2."""
import math
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

EPI_BIAS, EPI_ROWBIAS, EPI_RESID, EPI_ACCUM, EPI_MASK, EPI_LRELU2, EPI_TANH, EPI_F32OUT, EPI_NO_C, EPI_RESID_INV = \
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512
EPI_MASKBITS, EPI_BITS2 = 1024, 2048
EPI_SOFTBWD, EPI_GEGLU, EPI_LNFOLD = 4096, 8192, 16384
FLAG_NAMES = {"BIAS": EPI_BIAS, "ROWBIAS": EPI_ROWBIAS, "RESID": EPI_RESID, "ACCUM": EPI_ACCUM, "MASK": EPI_MASK, "LRELU2": EPI_LRELU2,
              "TANH": EPI_TANH, "F32OUT": EPI_F32OUT, "NO_C": EPI_NO_C, "RESID_INV": EPI_RESID_INV, "MASKBITS": EPI_MASKBITS,
              "BITS2": EPI_BITS2, "SOFTBWD": EPI_SOFTBWD, "GEGLU": EPI_GEGLU, "LNFOLD": EPI_LNFOLD}
U32 = 2.0 ** -24
SENT16 = 0x7B7B                      # untouched 16-bit elements (finite in fp16 and bf16)
SENT32 = 0x7B7B7B7B                  # untouched fp32 elements
SENT8 = 0xAA                         # untouched bytes of a sign-bit tensor
# tile configuration -> (BM, BN); 3 .. 6 are the register-staged kernel, the others LDS-DMA tiles (csrc/gemm_conv.hip launch_by_cfg)
TILES = {1: (256, 256), 2: (256, 128), 3: (128, 128), 4: (128, 64), 5: (128, 32), 6: (64, 64), 7: (320, 256), 8: (192, 256),
         9: (320, 128), 10: (192, 128), 11: (128, 128), 12: (64, 64), 13: (128, 64), 14: (64, 128), 15: (64, 64), 16: (64, 128),
         17: (128, 64), 18: (128, 128), 19: (512, 128)}
DMA_TILES = [t for t in TILES if not 3 <= t <= 6]
LN_TILES = [1, 2, 10, 11, 18, 12, 13, 14, 3, 4, 6]       # what dmx_gemm_launch_ln maps onto distinct instantiations
INT_FIELDS = ("M N K ldw Hi Wi Ci lda Hq Wq sy sx ntaps Ho Wo ldc osy ooy osx oox ldr ldx ldc2 Z Zi sAo sAi sWo sWi sCo sCi flags tile_cfg "
              "ldrb nslots ldxb ldb2").split()
FLOAT_FIELDS = "alpha act_slope mask_slope resid_inv_slope ln_eps".split()
PTR_FIELDS = "A W C C2 bias rowbias R X colsum rowstats_in XB B2".split()


def act_eps(adt):
    return torch.finfo(adt).eps / 2


def act_tiny(adt):
    return torch.finfo(adt).smallest_normal * torch.finfo(adt).eps


def launch(**kw):
    """One descriptor: integer / float fields as in GemmDesc, pointer fields as NAMES of buffers of the case, tdy / tdx as lists."""
    d = {k: 0 for k in INT_FIELDS}
    d.update({k: 0.0 for k in FLOAT_FIELDS})
    d.update({k: None for k in PTR_FIELDS})
    d.update(Z=1, Zi=1, sy=1, sx=1, osy=1, osx=1, alpha=1.0, tdy=[0], tdx=[0], bias_first=None)     # bias_first: emulate() only (None: its rule)
    unknown = set(kw) - set(d)
    assert not unknown, unknown
    d.update(kw)
    L = SimpleNamespace(**d)
    assert L.K == L.ntaps * L.Ci and len(L.tdx) == L.ntaps and len(L.tdy) == L.ntaps
    return L


class Buf:
    """A flat buffer.  kind: 'act' (16-bit), 'f32' or 'bits' (a sign-bit tensor: one BYTE per 8 channels, bit e of byte k <=> channel
    8 k + e > 0, csrc/dmx_common.h EPI_MASKBITS; data holds the byte values 0 .. 255).  data: float64 values; NaN marks a sentinel
    element (outputs only)."""

    def __init__(self, kind, data):
        self.kind = kind
        self.data = data.double().reshape(-1).clone()

    def rounded(self, adt):
        if adt is None or self.kind == "bits":
            return Buf(self.kind, self.data)
        return Buf(self.kind, (self.data.to(adt) if self.kind == "act" else self.data.float()).double())


def sentinel(kind, n):
    return Buf(kind, torch.full((n,), float("nan"), dtype=torch.float64))


_BITW = 2.0 ** torch.arange(8, dtype=torch.float64)


def pack_bits(pos):
    """(rows, N) bool, N % 8 == 0 -> (rows, N / 8) byte values (float64): bit e of byte k <=> column 8 k + e"""
    return (pos.double().view(pos.shape[0], -1, 8) * _BITW).sum(-1)


def unpack_bits(by, reverse=False):
    """(rows, N / 8) byte values -> (rows, N) bool"""
    e = torch.arange(8)
    b = (by.long()[:, :, None] >> (7 - e if reverse else e)) & 1
    return b.view(by.shape[0], -1) > 0


# ------------------------------------------------------------------------------------------------------------------ the model
def _rows(L):
    m = torch.arange(L.M)
    P = L.Hq * L.Wq
    b = m // P
    rem = m - b * P
    qy = rem // L.Wq
    qx = rem - qy * L.Wq
    return b, qy, qx


def gather(L, bufs, z):
    """A_gather (M, K) and W (N, K) of batch z, float64."""
    b, qy, qx = _rows(L)
    zo, zi = z // L.Zi, z % L.Zi
    A = bufs[L.A].data
    cols = []
    c = torch.arange(L.Ci)
    for t in range(L.ntaps):
        iy, ix = qy * L.sy + L.tdy[t], qx * L.sx + L.tdx[t]
        ok = (iy >= 0) & (iy < L.Hi) & (ix >= 0) & (ix < L.Wi)
        pix = (b * L.Hi + iy.clamp(0, L.Hi - 1)) * L.Wi + ix.clamp(0, L.Wi - 1)
        idx = zo * L.sAo + zi * L.sAi + pix[:, None] * L.lda + c[None, :]
        cols.append(torch.where(ok[:, None], A[idx], torch.zeros((), dtype=torch.float64)))
    Ag = torch.cat(cols, 1)
    widx = zo * L.sWo + zi * L.sWi + torch.arange(L.N)[:, None] * L.ldw + torch.arange(L.K)[None, :]
    return Ag, bufs[L.W].data[widx]


def out_rows(L):
    b, qy, qx = _rows(L)
    return (b * L.Ho + qy * L.osy + L.ooy) * L.Wo + qx * L.osx + L.oox, b


def _gelu(g):
    return 0.5 * g * torch.special.erfc(-g / math.sqrt(2.0))          # = g / 2 (1 + erf(g / sqrt 2)), free of cancellation


def _dgelu(g):
    return 0.5 * torch.special.erfc(-g / math.sqrt(2.0)) + g * torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)


def _sup_dgelu(lo, hi):
    """sup |gelu'| over [lo, hi]: gelu'' = phi(x) (2 - x^2) changes sign only at +-sqrt 2, so the sup sits at an end or at one of those"""
    s = torch.maximum(_dgelu(lo).abs(), _dgelu(hi).abs())
    for c in (-math.sqrt(2.0), math.sqrt(2.0)):
        inside = (lo < c) & (hi > c)
        s = torch.where(inside, torch.maximum(s, _dgelu(torch.tensor(c, dtype=torch.float64)).abs()), s)
    return s


def geglu_cols(N):
    """packed columns of the values of output column j = 16 b + c: 32 b + c; its gate sits 16 further (layers.hip geglu_src_row)"""
    j = torch.arange(N // 2)
    return 32 * (j // 16) + j % 16


def geglu_src_row(p, half):
    b, q = p >> 5, p & 31
    return 16 * b + q if q < 16 else half + 16 * b + (q - 16)


def ln_stats(L, bufs, Ag):
    """exact (mean, rstd) of the 16-bit rows and the bound terms (d_mean, d_rstd)"""
    K, ns = L.K, L.nslots
    mean = Ag.sum(1) / K
    q = (Ag * Ag).sum(1)
    var = (q / K - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + L.ln_eps)
    d_mean = (ns + 2) * U32 * Ag.abs().sum(1) / K
    d_var = (ns + 3) * U32 * q / K + 2 * mean.abs() * d_mean + 3 * U32 * mean * mean
    d_rstd = rstd * (d_var / (2 * (var + L.ln_eps)) + 4 * U32)
    return mean, rstd, d_mean, d_rstd


def run_launch(L, state, adt, mut=None, in_err=None):
    """Float64 model of one launch.  state: {name: Buf} with the CURRENT contents of every buffer (EPI_ACCUM reads C).
    -> list of writes (buffer name, flat indices (M', N'), exact values, bound): the set of elements the launch may write.
    adt: output type for the bound (None: bounds are zeros).  mut: name of a mutant of the reference.
    EPI_BITS2 adds a write to the 'bits' buffer B2: (name, byte indices (M', N / 8), byte of (ref > 0), byte of the bits that are FREE
    when no 16-bit tensor is stored next to them: |ref| <= A + tiny, the sign of what the kernel holds is open there).
    in_err: {buffer name: flat element-wise bound of what that buffer's holder may differ from state by} for the input A (the
    intermediate of a fused pair, tests/pair_cases.py): P = gather(in_err) |W|^T joins the bound like the accumulators themselves."""
    fl = L.flags
    writes = []
    eps, tiny = (act_eps(adt), act_tiny(adt)) if adt is not None else (0.0, 0.0)
    for z in range(L.Z):
        zo, zi = z // L.Zi, z % L.Zi
        coff = zo * L.sCo + zi * L.sCi
        Ag, Wm = gather(L, state, z)
        if mut == "skip_k_chunk":
            Ag = Ag.clone()
            Ag[:, L.K - 8:] = 0.0
        if mut == "drop_last_tap":
            Ag = Ag.clone()
            Ag[:, L.K - L.Ci:] = 0.0
        acc = Ag @ Wm.t()
        S = Ag.abs() @ Wm.abs().t()
        P_in = None
        if in_err is not None and L.A in in_err:
            Eg, _ = gather(L, {**state, L.A: Buf("act", in_err[L.A])}, z)
            P_in = Eg @ Wm.abs().t()
            S = S + P_in
        orow, b = out_rows(L)
        if mut == "oox_off_by_one":
            orow = orow + 1
        n = torch.arange(L.N)
        E = 0
        pre = torch.zeros_like(acc) if P_in is None else P_in     # error terms that are not of the form (K + E) u32 S

        def at(name, ld, rows=orow, off=coff):
            return state[name].data[off + rows[:, None] * ld + n[None, :]]

        v = acc
        if fl & EPI_LNFOLD:
            mean, rstd, d_mean, d_rstd = ln_stats(L, state, Ag)
            cs = state[L.colsum].data[n]
            bs = state[L.bias].data[n] if L.bias else torch.zeros(L.N, dtype=torch.float64)
            if mut == "geglu_bias_unpacked":
                bs = _unpack_bias(bs)
            mc = mean[:, None] * cs[None, :]
            t = acc - mc
            d_t = 2 * L.K * U32 * S + cs.abs()[None, :] * d_mean[:, None] + 3 * U32 * mc.abs() + U32 * t.abs()
            v = rstd[:, None] * t + bs[None, :]
            pre = rstd[:, None] * d_t + t.abs() * d_rstd[:, None] + 2 * U32 * ((rstd[:, None] * t).abs() + bs.abs()[None, :])
            S = torch.zeros_like(S)
            Ssub = (rstd[:, None] * t).abs() + bs.abs()[None, :]       # magnitude carried into the later fp32 operations
        else:
            Ssub = None
        if fl & EPI_MASK:
            x = at(L.X, L.ldx)
            pos = (x >= 0) if mut == "mask_zero_positive" else (x > 0)
            f = torch.where(pos, 1.0, L.mask_slope)
            v, S, pre = v * f, S * f, pre * f
            E += 1
        if fl & EPI_MASKBITS:                               # EPI_MASK with the factor taken from the bit
            by = state[L.XB].data[orow[:, None] * L.ldxb + torch.arange(L.N // 8)[None, :]]
            f = torch.where(unpack_bits(by, reverse=(mut == "mask_bit_reversed")), 1.0, L.mask_slope)
            v, S, pre = v * f, S * f, pre * f
            E += 1
        if fl & EPI_SOFTBWD:
            delta = state[L.rowbias].data[z * L.M + torch.arange(L.M)]
            x = at(L.X, L.ldx)
            v = (v - delta[:, None]) * x
            S = (S + delta.abs()[:, None]) * x.abs()
            E += 2
        if (fl & EPI_BIAS) and not (fl & EPI_LNFOLD):
            bb = state[L.bias].data[n]
            if mut == "geglu_bias_unpacked":
                bb = _unpack_bias(bb)
            v, S = v + bb[None, :], S + bb.abs()[None, :]
            E += 1
        if fl & EPI_ROWBIAS:
            bi = b
            if mut == "rowbias_neighbour":              # the image of the fragment's first row for all 16 rows of the fragment
                m = torch.arange(L.M)
                bi = (m // 16 * 16) // (L.Hq * L.Wq)
            rb = state[L.rowbias].data[bi[:, None] * (L.ldrb or L.N) + n[None, :]]
            v, S = v + rb, S + rb.abs()
            E += 1
        if Ssub is not None:
            S = S + Ssub
        Kacc = 0 if fl & EPI_LNFOLD else L.K                # (the fold's accumulation error sits in `pre`)
        if fl & EPI_GEGLU:
            A = pre + 2 * (Kacc + E) * U32 * S
            vc = geglu_cols(L.N)
            gc = vc + 16
            if mut == "geglu_swap":
                vc, gc = gc, vc
            val, g, Av, Ag_ = v[:, vc], v[:, gc], A[:, vc], A[:, gc]
            if mut == "geglu_erf_fp32":                     # the cancelling form, evaluated in fp32
                gf = g.float()
                ge = (0.5 * gf * (1.0 + torch.erf(gf * 0.70710678118654752))).double()
            else:
                ge = _gelu(g)
            sup = _sup_dgelu(g - Ag_, g + Ag_)
            v = val * ge
            # (+ two fp32 products)
            pre = _gelu(g).abs() * Av + val.abs() * sup * Ag_ + Av * Ag_ * sup + 2 * 2 * U32 * (val * _gelu(g)).abs()
            S, E, Kacc = torch.zeros_like(v), 0, 0
            n = torch.arange(L.N // 2)
        if fl & EPI_RESID:
            r = at(L.R, L.ldr)
            E += 1
            if fl & EPI_RESID_INV:
                E += 1
                if mut != "resid_no_inv":
                    r = torch.where(r > 0, r, r * L.resid_inv_slope)
            v, S = v + r, S + r.abs()
        if mut == "alpha_after_accum" and (fl & EPI_ACCUM):
            v = (v + at(L.C, L.ldc)) * L.alpha
        else:
            if L.alpha != 1.0:
                v, S, pre = v * L.alpha, S * abs(L.alpha), pre * abs(L.alpha)
                E += 1
            if fl & EPI_ACCUM:
                pc = at(L.C, L.ldc)
                v, S = v + pc, S + pc.abs()
                E += 1
        if fl & EPI_TANH:
            v = torch.tanh(v)                               # |tanh'| <= 1: A is carried unchanged
            E += 1
        A = pre + 2 * (Kacc + E) * U32 * S
        rows, cols = slice(None), slice(None)
        if mut == "drop_last_row":
            rows = slice(0, L.M - 1)
        if mut == "drop_last_chunk":
            cols = slice(0, n.numel() - 8)

        def bound(ref, kind):
            if adt is None:
                return torch.zeros_like(ref)
            return A + (4 * U32 * ref.abs() if kind == "f32" else 1.5 * eps * ref.abs() + tiny / 2)

        def bits_write(ref, A_):
            free = (ref.abs() <= A_ + tiny) if adt is not None else torch.zeros_like(ref, dtype=torch.bool)
            bidx = orow[:, None] * L.ldb2 + torch.arange(L.N // 8)[None, :]
            writes.append((L.B2, bidx[rows], pack_bits(ref > 0)[rows], pack_bits(free)[rows]))

        if not (fl & EPI_NO_C):
            idx = coff + orow[:, None] * L.ldc + n[None, :]
            writes.append((L.C, idx[rows, cols], v[rows, cols], bound(v, state[L.C].kind)[rows, cols]))
            if (fl & EPI_BITS2) and not (fl & EPI_LRELU2):
                bits_write(v, A)
        if fl & EPI_LRELU2:
            v2 = torch.where(v > 0, v, v * L.act_slope)
            idx = coff + orow[:, None] * L.ldc2 + n[None, :]
            if adt is not None:                             # the slope carries A wherever the sign of v is beyond doubt (|v| > A)
                A = A * torch.where((v < 0) & (v.abs() > A), L.act_slope, 1.0) + U32 * v2.abs()
            if L.C2 is not None:
                writes.append((L.C2, idx[rows, cols], v2[rows, cols], bound(v2, "act")[rows, cols]))
            if fl & EPI_BITS2:
                bits_write(v2, A)
    return writes


def _unpack_bias(bp):
    """what a kernel adds that reads the PACKED bias array as if it were [values | gates]"""
    N = bp.numel()
    return bp[torch.tensor([geglu_src_row(p, N // 2) for p in range(N)])]


def expected(launches, bufs, adt, mut=None):
    """Run every launch of a case.  -> {output buffer name: (values, bound, count)}: flat float64 values (NaN = sentinel kept), the
    element-wise bound and how many launches wrote each element (0 = must keep its sentinel)."""
    return expected_all(launches, bufs, adt, mut)[0]


def expected_all(launches, bufs, adt, mut=None, run=run_launch):
    """-> (outs as expected() returns them for the 16-bit / fp32 outputs, the same for the sign-bit outputs: {B2 name: (byte of
    (ref > 0), byte of the free bits, count)}).  An EPI_ACCUM launch onto elements an EARLIER launch of the case wrote inherits that
    launch's bound (its input is the other's output)."""
    state = {k: Buf(b.kind, b.data) for k, b in bufs.items()}
    outs = {}
    for L in launches:
        for name in (L.C, L.C2, L.B2):
            if name is not None and name not in outs:
                nel = state[name].data.numel()
                outs[name] = (state[name].data, torch.zeros(nel, dtype=torch.float64), torch.zeros(nel, dtype=torch.int64))
    for L in launches:
        for name, idx, ref, bnd in run(L, state, adt, mut):
            val, bd, cnt = outs[name]
            idx = idx.reshape(-1)
            ok = (idx >= 0) & (idx < val.numel())          # (a mutant's row map may leave the buffer)
            val[idx[ok]] = ref.reshape(-1)[ok]
            carry = bd[idx[ok]] if (L.flags & EPI_ACCUM) and name == L.C else 0.0
            bd[idx[ok]] = bnd.reshape(-1)[ok] + carry
            cnt[idx[ok]] += 1
    return ({k: v for k, v in outs.items() if state[k].kind != "bits"}, {k: v for k, v in outs.items() if state[k].kind == "bits"})


def bits_source(launches):
    """{B2 name: (name of the 16-bit tensor stored next to it, its row stride, the B2 row stride, N)} -- None where the bits leave alone"""
    src = {}
    for L in launches:
        if L.flags & EPI_BITS2:
            if L.flags & EPI_LRELU2:
                src[L.B2] = (L.C2, L.ldc2, L.ldb2, L.N) if L.C2 is not None else None
            else:
                src[L.B2] = (L.C, L.ldc, L.ldb2, L.N) if not (L.flags & EPI_NO_C) else None
    return src


def check_bits(name, got_bytes, exp_bits, src, stored):
    """The third kind of write, compared EXACTLY.  got_bytes: flat byte values of B2 after the launches (float64 / int); exp_bits: its
    entry of expected_all()[1]; src: its entry of bits_source(); stored: flat float64 values of the stored 16-bit tensor (src not None).
    -> number of wrong bytes among the written ones (the caller asserts 0 and checks the unwritten ones against the sentinel)."""
    ref, free, cnt = exp_bits
    w = cnt > 0
    got = got_bytes.long()
    if src is not None:                                     # the sign bits of what the kernel itself stored, element for element
        _, ld, ldb2, N = src
        rows = stored.numel() // ld
        want = torch.full_like(ref, -1.0)
        nb_rows = min(rows, ref.numel() // ldb2)
        wb = pack_bits(stored.view(rows, ld)[:nb_rows, :N] > 0)
        want.view(-1)[:nb_rows * ldb2].view(nb_rows, ldb2)[:, :N // 8] = wb
        return int((got[w] != want.long()[w]).sum())
    return int((((got[w] ^ ref.long()[w]) & ~free.long()[w] & 0xFF) != 0).sum())


def mutant_ratio(exp, mutd, exp_bits=None, mut_bits=None):
    """largest |mutant - ref| / bound over what the reference writes; inf where a mutant leaves a sentinel in the writable set or
    writes outside it, or where a sign byte differs outside the free bits of either side"""
    worst = 0.0
    for name, (ref, free, cnt) in (exp_bits or {}).items():
        mref, mfree, mc = mut_bits[name]
        w = cnt > 0
        if ((mc > 0) != w).any():
            return float("inf")
        if (((ref.long()[w] ^ mref.long()[w]) & ~(free.long()[w] | mfree.long()[w]) & 0xFF) != 0).any():
            return float("inf")
    for name, (val, bd, cnt) in exp.items():
        mv, _, mc = mutd[name]
        w = cnt > 0
        if ((mc > 0) & ~w).any():
            return float("inf")
        if not w.any():
            continue
        r = (mv[w] - val[w]).abs() / bd[w]
        r[torch.isnan(r)] = float("inf")
        worst = max(worst, r.max().item())
    return worst


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation
def _acc32(Ag, Wm, order, init=None):
    a, w = Ag.float(), Wm.float()                         # 16-bit operands: exact in fp32, and so is every product
    acc = torch.zeros(a.shape[0], w.shape[0]) if init is None else init.float()[None, :].expand(a.shape[0], -1).clone()
    K = a.shape[1]
    if order == "seq":
        for k in range(K):
            acc = acc + a[:, k:k + 1] * w[None, :, k]
    else:                                                 # one MFMA: 32 products summed (exactly here), then one add to the accumulator
        for k in range(0, K, 32):
            acc = acc + (Ag[:, k:k + 32] @ Wm[:, k:k + 32].t()).float()
    return acc


def emulate(launches, bufs, adt, order):
    """fp32 emulation of the kernels' arithmetic on the rounded buffers: fp32 accumulation (order 'seq' or 'blk32'), accumulators
    started at the bias where nothing precedes it (EPI_BIASINIT), split-K slices added before the epilogue, the fp32 epilogue, for the
    LayerNorm fold fp32 slot sums and ln_apply's fma, and ONE rounding to the output type.  -> {name: flat float64 values}"""
    state = {k: Buf(b.kind, b.data) for k, b in bufs.items()}
    f32 = torch.float32
    for L in launches:
        fl = L.flags
        for z in range(L.Z):
            coff = (z // L.Zi) * L.sCo + (z % L.Zi) * L.sCi
            Ag, Wm = gather(L, state, z)
            orow, b = out_rows(L)
            n = torch.arange(L.N)

            def at(name, ld):
                return state[name].data[coff + orow[:, None] * ld + n[None, :]].float()

            slices = L.tile_cfg // 100 if L.tile_cfg >= 100 else 1
            bias_first = bool(fl & EPI_BIAS) and not (fl & (EPI_MASK | EPI_MASKBITS | EPI_SOFTBWD | EPI_LNFOLD)) and slices == 1
            if L.bias_first is not None:
                bias_first = bool(fl & EPI_BIAS) and L.bias_first
            if slices > 1:
                nk = -(-L.K // 64)
                per = -(-nk // slices)
                parts = [_acc32(Ag[:, s * per * 64:(s + 1) * per * 64], Wm[:, s * per * 64:(s + 1) * per * 64], order)
                         for s in range(slices) if s * per * 64 < L.K]
                v = parts[0]
                for p in parts[1:]:
                    v = v + p
            else:
                v = _acc32(Ag, Wm, order, state[L.bias].data[n] if bias_first else None)
            if fl & EPI_LNFOLD:
                ns = L.nslots
                st = state[L.rowstats_in].data.float().view(L.M, ns, 2)
                si, qi = torch.zeros(L.M), torch.zeros(L.M)
                for s in range(ns):
                    si, qi = si + st[:, s, 0], qi + st[:, s, 1]
                inv_c = torch.tensor(1.0 / L.K, dtype=f32)
                mean = si * inv_c
                rstd = 1.0 / torch.sqrt((qi * inv_c - mean * mean).clamp_min(0.0) + torch.tensor(L.ln_eps, dtype=f32))
                t = v - mean[:, None] * state[L.colsum].data[n].float()[None, :]
                bs = state[L.bias].data[n] if L.bias else torch.zeros(L.N, dtype=torch.float64)
                v = (rstd.double()[:, None] * t.double() + bs[None, :]).float()                    # fma: one rounding
            if fl & EPI_MASK:
                v = v * torch.where(at(L.X, L.ldx) > 0, torch.tensor(1.0), torch.tensor(L.mask_slope, dtype=f32))
            if fl & EPI_MASKBITS:
                by = state[L.XB].data[orow[:, None] * L.ldxb + torch.arange(L.N // 8)[None, :]]
                v = v * torch.where(unpack_bits(by), torch.tensor(1.0), torch.tensor(L.mask_slope, dtype=f32))
            if fl & EPI_SOFTBWD:
                v = (v - state[L.rowbias].data[z * L.M + torch.arange(L.M)].float()[:, None]) * at(L.X, L.ldx)
            if (fl & EPI_BIAS) and not bias_first and not (fl & EPI_LNFOLD):
                v = v + state[L.bias].data[n].float()[None, :]
            if fl & EPI_ROWBIAS:
                v = v + state[L.rowbias].data[b[:, None] * (L.ldrb or L.N) + n[None, :]].float()
            if fl & EPI_GEGLU:
                vc = geglu_cols(L.N)
                g = v[:, vc + 16]
                v = v[:, vc] * (0.5 * g * torch.special.erfc(g * -0.70710678118654752))
                n = torch.arange(L.N // 2)
            if fl & EPI_RESID:
                r = at(L.R, L.ldr)
                if fl & EPI_RESID_INV:
                    r = torch.minimum(r, r * torch.tensor(L.resid_inv_slope, dtype=f32))
                v = v + r
            if L.alpha != 1.0:
                v = v * torch.tensor(L.alpha, dtype=f32)
            if fl & EPI_ACCUM:
                v = v + at(L.C, L.ldc)
            if fl & EPI_TANH:
                v = torch.tanh(v)
            assert v.dtype == f32

            def bits_out(o16):                          # the sign bits of the 16-bit value the kernel holds
                bidx = orow[:, None] * L.ldb2 + torch.arange(L.N // 8)[None, :]
                state[L.B2].data[bidx.reshape(-1)] = pack_bits(o16.double() > 0).reshape(-1)

            if not (fl & EPI_NO_C):
                o = v if state[L.C].kind == "f32" else v.to(adt)
                state[L.C].data[(coff + orow[:, None] * L.ldc + n[None, :]).reshape(-1)] = o.double().reshape(-1)
                if (fl & EPI_BITS2) and not (fl & EPI_LRELU2):
                    bits_out(o)
            if fl & EPI_LRELU2:
                v2 = torch.maximum(v, v * torch.tensor(L.act_slope, dtype=f32)).to(adt)
                if L.C2 is not None:
                    state[L.C2].data[(coff + orow[:, None] * L.ldc2 + n[None, :]).reshape(-1)] = v2.double().reshape(-1)
                if fl & EPI_BITS2:
                    bits_out(v2)
    return {k: state[k].data for L in launches for k in (L.C, L.C2, L.B2) if k is not None}


# ------------------------------------------------------------------------------------------------------------------ builders
# Each returns (launches, bufs) with float64 UNROUNDED operands (Buf.rounded(adt) rounds them) and, as `torch_ref`, a function that
# computes the same outputs with torch's own float64 operators from the same unrounded operands -> {buffer name: logical tensor}.
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _epi_bufs(g, bufs, L, rows, N, flags, n_img, ld_pad, kind="act", special_mask=False):
    """side tensors and outputs of an epilogue flag set for `rows` output rows of N columns; every ld is N + ld_pad"""
    ld = N + ld_pad
    kw = dict(ldc=ld, ldr=ld, ldx=ld, ldc2=ld, flags=flags)
    nel = rows * ld
    if flags & EPI_BIAS:
        bufs["bias"] = Buf("f32", torch.randn(N, generator=g))
        kw["bias"] = "bias"
    if flags & EPI_ROWBIAS:
        ldrb = N + 4
        bufs["rowbias"] = Buf("f32", torch.randn(n_img * ldrb, generator=g))
        kw.update(rowbias="rowbias", ldrb=ldrb)
    if flags & EPI_RESID:
        bufs["R"] = Buf("act", torch.randn(nel, generator=g))
        kw["R"] = "R"
    if flags & EPI_RESID_INV:
        kw["resid_inv_slope"] = 10.0
    if flags & EPI_MASK:
        x = torch.randn(nel, generator=g)
        if special_mask:                                # +0, -0 and subnormals of either sign in the mask source
            tiny = act_tiny(torch.float16)
            sp = torch.tensor([0.0, -0.0, tiny, -tiny, 3 * tiny, -5 * tiny, 0.0, -0.0])
            pos = torch.randperm(nel, generator=g)[:nel // 4]
            x[pos] = sp[torch.arange(pos.numel()) % 8]
        bufs["X"] = Buf("act", x)
        kw.update(X="X", mask_slope=0.1)
    if flags & EPI_LRELU2:
        bufs["C2"] = sentinel("act", nel)
        kw.update(C2="C2", act_slope=0.1)
    if flags & EPI_MASKBITS:                            # row strides wider than N / 8 (ldxb a multiple of 8: the tiles load words)
        ldxb = (N // 64 + 1) * 8
        bufs["XB"] = Buf("bits", torch.randint(0, 256, (rows * ldxb,), generator=g))
        kw.update(XB="XB", ldxb=ldxb, mask_slope=0.1)
    if flags & EPI_BITS2:
        ldb2 = N // 8 + 3
        bufs["B2"] = sentinel("bits", rows * ldb2)
        kw.update(B2="B2", ldb2=ldb2)
    bufs["C"] = sentinel(kind, nel)
    kw["C"] = "C"
    return kw


def _prev_c(g, bufs, launches):
    """EPI_ACCUM: the writable elements of C hold a previous value, all others the sentinel"""
    c = bufs["C"]
    for L in launches:
        for _, idx, _, _ in run_launch(SimpleNamespace(**{**vars(L), "flags": L.flags & ~(EPI_ACCUM | EPI_LRELU2 | EPI_NO_C)}),
                                       {**bufs, "C": Buf(c.kind, torch.zeros_like(c.data))}, None):
            idx = idx.reshape(-1)
            c.data[idx] = torch.randn(idx.numel(), generator=g).double()


def conv1d_case(name, B, T, Ci, Co, k, dil, flags, alpha=1.0, tile=0, ld_pad=8, M=None, kind="act", row_scale=None, special_mask=False):
    """dilated conv1d, 'same' padding, channels-last; M < B * T launches a partial last image (its other rows keep the sentinel)"""
    g = _gen(name)
    pad = (k * dil - dil) // 2
    x = torch.randn(B, T, Ci, generator=g).double()
    if row_scale is not None:
        x = x * row_scale
    w = (torch.randn(Co, Ci, k, generator=g) / (Ci * k) ** 0.5).double()
    bufs = {"A": Buf("act", x), "W": Buf("act", w.permute(0, 2, 1).reshape(Co, k * Ci))}
    kw = _epi_bufs(g, bufs, None, B * T, Co, flags, B, ld_pad, kind, special_mask)
    L = launch(A="A", W="W", M=M or B * T, N=Co, K=k * Ci, ldw=k * Ci, Hi=1, Wi=T, Ci=Ci, lda=Ci, Hq=1, Wq=T, ntaps=k, Ho=1, Wo=T,
               tdy=[0] * k, tdx=[t * dil - pad for t in range(k)], alpha=alpha, tile_cfg=tile, **kw)
    if flags & EPI_ACCUM:
        _prev_c(g, bufs, [L])

    def torch_ref(b):
        xx, ww = b["A"].data.view(B, T, Ci), b["W"].data.view(Co, k, Ci).permute(0, 2, 1)
        return F.conv1d(xx.transpose(1, 2), ww, None, padding=pad, dilation=dil).transpose(1, 2).reshape(B * T, Co)
    return [L], bufs, torch_ref


def convT1d_case(name, B, T, Ci, Co, k, s, p, flags=EPI_BIAS):
    """ConvTranspose1d as one launch per output phase r: osx = stride, oox = r, the taps j = (r + p) % s + i s (layers.hip conv_fwd_1d)"""
    g = _gen(name)
    To = (T - 1) * s - 2 * p + k
    x = torch.randn(B, T, Ci, generator=g).double()
    wt = (torch.randn(Ci, Co, k, generator=g) * (s / (Ci * k)) ** 0.5).double()
    bufs = {"A": Buf("act", x)}
    kw = _epi_bufs(g, bufs, None, B * To, Co, flags, B, 8)
    launches = []
    for r in range(s):
        taps = list(range((r + p) % s, k, s))
        nt, base = len(taps), (r + p) // s
        bufs[f"W{r}"] = Buf("act", wt[:, :, taps].permute(1, 2, 0).reshape(Co, nt * Ci))
        Wq = -(-(To - r) // s)
        launches.append(launch(A="A", W=f"W{r}", M=B * Wq, N=Co, K=nt * Ci, ldw=nt * Ci, Hi=1, Wi=T, Ci=Ci, lda=Ci, Hq=1, Wq=Wq, ntaps=nt,
                               Ho=1, Wo=To, osx=s, oox=r, tdy=[0] * nt, tdx=[base - i for i in range(nt)], **kw))

    def torch_ref(b):
        return F.conv_transpose1d(b["A"].data.view(B, T, Ci).transpose(1, 2), wt, None, stride=s, padding=p).transpose(1, 2).reshape(B * To, Co)
    return launches, bufs, torch_ref


def convT1d_dgrad_case(name, B, T, Ci, Co, k, s, p, flags=0):
    """dgrad of ConvTranspose1d: a stride-s walk over dout (sx = stride), all k taps, stride-1 output map (layers.hip conv_bwd_1d_desc)"""
    g = _gen(name)
    To = (T - 1) * s - 2 * p + k
    dout = torch.randn(B, To, Co, generator=g).double()
    wt = (torch.randn(Ci, Co, k, generator=g) * (s / (Co * k)) ** 0.5).double()
    bufs = {"A": Buf("act", dout), "W": Buf("act", wt.permute(0, 2, 1).reshape(Ci, k * Co))}
    kw = _epi_bufs(g, bufs, None, B * T, Ci, flags, B, 8)
    L = launch(A="A", W="W", M=B * T, N=Ci, K=k * Co, ldw=k * Co, Hi=1, Wi=To, Ci=Co, lda=Co, Hq=1, Wq=T, sx=s, ntaps=k, Ho=1, Wo=T,
               tdy=[0] * k, tdx=[t - p for t in range(k)], **kw)

    def torch_ref(b):
        x = torch.zeros(B, Ci, T, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose1d(x, wt, None, stride=s, padding=p)
        (gx,) = torch.autograd.grad(y, x, b["A"].data.view(B, To, Co).transpose(1, 2))
        return gx.transpose(1, 2).reshape(B * T, Ci)
    return [L], bufs, torch_ref


def conv2d_s2_case(name, B, H, W, Ci, Co, flags=EPI_BIAS):
    """3x3 convolution, stride 2, padding (0, 1): nothing before the image, one row / column after it (the diffusers downsampler)"""
    g = _gen(name)
    Ho, Wo = (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1
    x = torch.randn(B, H, W, Ci, generator=g).double()
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / (Ci * 9) ** 0.5).double()
    bufs = {"A": Buf("act", x), "W": Buf("act", w.permute(0, 2, 3, 1).reshape(Co, 9 * Ci))}
    kw = _epi_bufs(g, bufs, None, B * Ho * Wo, Co, flags, B, 8)
    L = launch(A="A", W="W", M=B * Ho * Wo, N=Co, K=9 * Ci, ldw=9 * Ci, Hi=H, Wi=W, Ci=Ci, lda=Ci, Hq=Ho, Wq=Wo, sy=2, sx=2, ntaps=9,
               Ho=Ho, Wo=Wo, tdy=[t // 3 for t in range(9)], tdx=[t % 3 for t in range(9)], **kw)

    def torch_ref(b):
        xx = F.pad(b["A"].data.view(B, H, W, Ci).permute(0, 3, 1, 2), (0, 1, 0, 1))
        return F.conv2d(xx, w, None, stride=2).permute(0, 2, 3, 1).reshape(B * Ho * Wo, Co)
    return [L], bufs, torch_ref


def _up2x_rows(p, t):
    return ([0] if t == 0 else [1, 2]) if p == 0 else ([0, 1] if t == 0 else [2])


def _up2x_delta(p, t):
    return t - 1 if p == 0 else t


def _up2x_wsum(w, py, px, ty, tx):
    return sum(w[:, :, ky, kx] for ky in _up2x_rows(py, ty) for kx in _up2x_rows(px, tx))          # (Co, Ci)


def up2x_fwd_case(name, B, H, W, Ci, Co, flags=EPI_BIAS):
    """nearest x2 upsampling + 3x3 / pad 1 convolution as four parity launches of 2x2 taps on the low-resolution image, the 3x3 weights
    that meet the same low-resolution pixel summed (layers.hip conv_up2x_fwd)"""
    g = _gen(name)
    x = torch.randn(B, H, W, Ci, generator=g).double()
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / (Ci * 9) ** 0.5).double()
    bufs = {"A": Buf("act", x)}
    kw = _epi_bufs(g, bufs, None, B * 4 * H * W, Co, flags, B, 8)
    launches = []
    for py in range(2):
        for px in range(2):
            ws = torch.stack([_up2x_wsum(w, py, px, ty, tx) for ty in range(2) for tx in range(2)], 1)      # (Co, 4, Ci)
            bufs[f"W{py}{px}"] = Buf("act", ws.reshape(Co, 4 * Ci))
            launches.append(launch(A="A", W=f"W{py}{px}", M=B * H * W, N=Co, K=4 * Ci, ldw=4 * Ci, Hi=H, Wi=W, Ci=Ci, lda=Ci, Hq=H, Wq=W,
                                   ntaps=4, Ho=2 * H, Wo=2 * W, osy=2, osx=2, ooy=py, oox=px,
                                   tdy=[_up2x_delta(py, ty) for ty in range(2) for tx in range(2)],
                                   tdx=[_up2x_delta(px, tx) for ty in range(2) for tx in range(2)], **kw))

    def torch_ref(b):
        xx = F.interpolate(b["A"].data.view(B, H, W, Ci).permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
        return F.conv2d(xx, w, None, padding=1).permute(0, 2, 3, 1).reshape(B * 4 * H * W, Co)
    return launches, bufs, torch_ref


def up2x_bwd_case(name, B, H, W, Ci, Co, flags=0):
    """its joint dgrad: 16 taps of a stride-2 walk over dout (layers.hip conv_up2x_bwd)"""
    g = _gen(name)
    dout = torch.randn(B, 2 * H, 2 * W, Co, generator=g).double()
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / (Co * 9) ** 0.5).double()
    taps = [(py, ty, px, tx) for py in range(2) for ty in range(2) for px in range(2) for tx in range(2)]
    wb = torch.stack([_up2x_wsum(w, py, px, ty, tx).t() for py, ty, px, tx in taps], 1)                   # (Ci, 16, Co)
    bufs = {"A": Buf("act", dout), "W": Buf("act", wb.reshape(Ci, 16 * Co))}
    kw = _epi_bufs(g, bufs, None, B * H * W, Ci, flags, B, 8)
    L = launch(A="A", W="W", M=B * H * W, N=Ci, K=16 * Co, ldw=16 * Co, Hi=2 * H, Wi=2 * W, Ci=Co, lda=Co, Hq=H, Wq=W, sy=2, sx=2, ntaps=16,
               Ho=H, Wo=W, tdy=[py - 2 * _up2x_delta(py, ty) for py, ty, px, tx in taps],
               tdx=[px - 2 * _up2x_delta(px, tx) for py, ty, px, tx in taps], **kw)

    def torch_ref(b):
        x = torch.zeros(B, Ci, H, W, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, None, padding=1)
        (gx,) = torch.autograd.grad(y, x, b["A"].data.view(B, 2 * H, 2 * W, Co).permute(0, 3, 1, 2))
        return gx.permute(0, 2, 3, 1).reshape(B * H * W, Ci)
    return [L], bufs, torch_ref


def conv2d_3x3_case(name, B, H, W, Ci, Co, flags, alpha=1.0, tile=0):
    """3x3 / pad 1 convolution (the split-K cases: K = 9 Ci)"""
    g = _gen(name)
    x = torch.randn(B, H, W, Ci, generator=g).double()
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / (Ci * 9) ** 0.5).double()
    bufs = {"A": Buf("act", x), "W": Buf("act", w.permute(0, 2, 3, 1).reshape(Co, 9 * Ci))}
    kw = _epi_bufs(g, bufs, None, B * H * W, Co, flags, B, 8, special_mask=True)
    L = launch(A="A", W="W", M=B * H * W, N=Co, K=9 * Ci, ldw=9 * Ci, Hi=H, Wi=W, Ci=Ci, lda=Ci, Hq=H, Wq=W, ntaps=9, Ho=H, Wo=W,
               tdy=[t // 3 - 1 for t in range(9)], tdx=[t % 3 - 1 for t in range(9)], alpha=alpha, tile_cfg=tile, **kw)

    def torch_ref(b):
        return F.conv2d(b["A"].data.view(B, H, W, Ci).permute(0, 3, 1, 2), w, None, padding=1).permute(0, 2, 3, 1).reshape(B * H * W, Co)
    return [L], bufs, torch_ref


def gemm_nt_case(name, Z, Zi, M, N, K, flags, tile=0, ld_pad=8, kind="act"):
    """plain (Z = 1) or batched NT GEMM: C[z] = A[z] W[z]^T, z = zo Zi + zi with outer / inner strides"""
    g = _gen(name)
    a = torch.randn(Z, M, K, generator=g).double()
    w = (torch.randn(Z, N, K, generator=g) / K ** 0.5).double()
    bufs = {"A": Buf("act", a), "W": Buf("act", w)}
    ld = N + ld_pad
    kw = _epi_bufs(g, bufs, None, Z * M, N, flags, 1, ld_pad, kind)
    L = launch(A="A", W="W", M=M, N=N, K=K, ldw=K, Hi=1, Wi=M, Ci=K, lda=K, Hq=1, Wq=M, ntaps=1, Ho=1, Wo=M, Z=Z, Zi=Zi,
               sAo=Zi * M * K, sAi=M * K, sWo=Zi * N * K, sWi=N * K, sCo=Zi * M * ld, sCi=M * ld, tile_cfg=tile, **kw)
    if flags & EPI_ACCUM:
        _prev_c(g, bufs, [L])

    def torch_ref(b):
        return (b["A"].data.view(Z, M, K) @ b["W"].data.view(Z, N, K).transpose(1, 2)).reshape(Z * M, N)
    return [L], bufs, torch_ref


def softbwd_case(name, Z, Nn, Cc, tile=1):
    """EPI_SOFTBWD: dS = P (dO V^T - delta) scale; P with whole zero rows, delta of either sign"""
    g = _gen(name)
    go = torch.randn(Z, Nn, Cc, generator=g).double()
    vv = torch.randn(Z, Nn, Cc, generator=g).double()
    P = torch.softmax(2.0 * torch.randn(Z, Nn, Nn, generator=g), -1).double()
    P[:, 5] = 0.0
    P[:, Nn - 1] = 0.0
    delta = torch.randn(Z, Nn, generator=g).double() * 3.0
    bufs = {"A": Buf("act", go), "W": Buf("act", vv), "X": Buf("act", P), "rowbias": Buf("f32", delta), "C": sentinel("act", Z * Nn * Nn)}
    L = launch(A="A", W="W", C="C", X="X", rowbias="rowbias", M=Nn, N=Nn, K=Cc, ldw=Cc, Hi=1, Wi=Nn, Ci=Cc, lda=Cc, Hq=1, Wq=Nn, ntaps=1,
               Ho=1, Wo=Nn, ldc=Nn, ldr=Nn, ldx=Nn, ldc2=Nn, Z=Z, Zi=1, sAo=Nn * Cc, sWo=Nn * Cc, sCo=Nn * Nn, flags=EPI_SOFTBWD,
               alpha=Cc ** -0.5, tile_cfg=tile)

    def torch_ref(b):
        dP = b["A"].data.view(Z, Nn, Cc) @ b["W"].data.view(Z, Nn, Cc).transpose(1, 2)
        return (b["X"].data.view(Z, Nn, Nn) * (dP - b["rowbias"].data.view(Z, Nn, 1)) * Cc ** -0.5).reshape(Z * Nn, Nn)
    return [L], bufs, torch_ref


def _geglu_gates(adt):
    """a 16-bit sweep of [-10, 10] (erf saturated at both ends), +0 / -0 and the subnormal range of the activation type"""
    adt = adt or torch.float16
    tiny, sn = act_tiny(adt), torch.finfo(adt).smallest_normal
    special = torch.tensor([0.0, -0.0, 10.0, -10.0, tiny, -tiny, 3 * tiny, -5 * tiny, 0.5 * sn, -0.75 * sn])
    return torch.cat([torch.linspace(-10.0, 10.0, 263), special]).to(adt).double()


def geglu_case(name, M, K, N, tile, ln=False, exact_gate_adt=False, adt=None, ld_pad=8):
    """feed-forward first projection with GEGLU in its epilogue: natural weights [N / 2 value rows | N / 2 gate rows] packed in blocks of
    32 = 16 values | their 16 gates, the bias packed alike (layers.hip geglu_src_row); ln: LayerNorm of the rows folded in (gamma into W,
    beta into the bias, colsum and the rows' slot sums as operands)"""
    g = _gen(name)
    half = N // 2
    src = torch.tensor([geglu_src_row(p, half) for p in range(N)])
    w = (torch.randn(N, K, generator=g) / K ** 0.5).double()
    bias = torch.randn(N, generator=g).double() * 0.5
    if exact_gate_adt:
        gates = _geglu_gates(adt)
        M = gates.numel()
        x = torch.randn(M, K, generator=g).double()
        x[:, 0] = gates
        w[:half, 0] = 0.0                                # value rows do not see column 0 ...
        w[half:] = 0.0
        w[half:, 0] = 1.0                                # ... gate rows see nothing else: the gate accumulators are exact
        flags = EPI_GEGLU
    else:
        scale = torch.logspace(math.log10(0.05), math.log10(4.0), M).double()
        scale[-(M // 4):] = 4.0                          # enough rows at the top for gates beyond +-10
        scale = scale[torch.randperm(M, generator=g)]
        x = torch.randn(M, K, generator=g).double() * scale[:, None]
        flags = EPI_GEGLU | EPI_BIAS
    bufs = {"A": Buf("act", x), "C": sentinel("act", M * (half + ld_pad))}
    kw = dict(A="A", W="W", C="C", M=M, N=N, K=K, ldw=K, Hi=1, Wi=M, Ci=K, lda=K, Hq=1, Wq=M, ntaps=1, Ho=1, Wo=M, ldc=half + ld_pad,
              tile_cfg=tile)
    if flags & EPI_BIAS:
        kw["bias"] = "bias"
    gamma = beta = None
    if ln:
        flags |= EPI_LNFOLD
        gamma, beta = (0.5 + torch.rand(K, generator=g)).double(), (0.3 * torch.randn(K, generator=g)).double()
        x = x / scale[:, None] * (0.5 + 2.0 * torch.rand(M, 1, generator=g).double())                       # LN is scale-free: moderate rows ...
        x = x - x.mean(1, keepdim=True)
        x = x + x.std(1, keepdim=True) * (2.0 * torch.rand(M, 1, generator=g).double() - 1.0) * 0.6           # ... with |mean| <= 0.6 std
        bufs["A"] = Buf("act", x)
        bufs["W"] = Buf("act", (w * gamma[None, :])[src])
        bufs["bias"] = Buf("f32", (2.0 * bias + w @ beta)[src])          # (a unit-variance bias: fewer values and gates at the level of A)
        ns = -(-K // 32)
        kw.update(colsum="colsum", rowstats_in="rowstats", nslots=ns, ln_eps=1e-5)
    else:
        bufs["W"] = Buf("act", w[src])
        bufs["bias"] = Buf("f32", bias[src])
    L = launch(flags=flags, **kw)

    def torch_ref(b):
        xx = b["A"].data.view(M, K)
        if ln:
            xx = F.layer_norm(xx, (K,), gamma, beta, 1e-5)
        h = xx @ w.t() + ((2.0 * bias if ln else bias) if flags & EPI_BIAS else 0.0)
        return h[:, :half] * F.gelu(h[:, half:])
    return [L], bufs, torch_ref


def finish_ln(bufs, L):
    """colsum and the slot sums are OPERANDS derived from the rounded A and W (what pack_layer and an EPI_ROWSTATS producer write)"""
    if not (L.flags & EPI_LNFOLD):
        return
    bufs["colsum"] = Buf("f32", bufs["W"].data.view(L.N, L.K).sum(1))
    x = bufs["A"].data.view(L.M, L.K)
    xp = F.pad(x, (0, L.nslots * 32 - L.K)).view(L.M, L.nslots, 32)
    bufs["rowstats"] = Buf("f32", torch.stack([xp.sum(-1), (xp * xp).sum(-1)], -1))


# ------------------------------------------------------------------------------------------------------------------ case table
class Case:
    """name, family, the builder and what the table test asks about: tile, flags, features."""

    def __init__(self, name, family, build, tile=0, flags=0, **feat):
        self.name, self.family, self._build, self.tile, self.flags, self.feat = name, family, build, tile, flags, feat
        self._cache = {}

    def data(self, adt):
        """(launches, bufs rounded to adt -- None: unrounded float64 --, torch_ref)"""
        if adt not in self._cache:
            launches, bufs, tref = self._build(adt)
            bufs = {k: b.rounded(adt) for k, b in bufs.items()}
            for L in launches:
                finish_ln(bufs, L)
            if adt is not None:
                bufs = {k: b.rounded(adt) for k, b in bufs.items()}
            self._cache[adt] = (launches, bufs, tref)
        return self._cache[adt]

    def expected(self, adt, mut=None):
        return self._expected(adt, mut)[0]

    def expected_bits(self, adt, mut=None):
        """the sign-bit outputs: {B2 name: (byte of (ref > 0), byte of the free bits, count)}"""
        return self._expected(adt, mut)[1]

    def _expected(self, adt, mut):
        key = ("exp", adt, mut)
        if key not in self._cache:
            launches, bufs, _ = self.data(adt)
            self._cache[key] = expected_all(launches, bufs, adt, mut)
        return self._cache[key]


F1 = EPI_BIAS | EPI_ROWBIAS | EPI_RESID
F2 = EPI_MASK | EPI_RESID | EPI_ACCUM
F3 = EPI_BIAS | EPI_RESID | EPI_RESID_INV | EPI_LRELU2
FLAG_SETS = {"bias-rowbias-resid": (F1, 0.5), "mask-resid-accum": (F2, 1.0), "bias-residinv-lrelu2": (F3, 1.0),
             "bias-residinv-lrelu2-noc": (F3 | EPI_NO_C, 1.0), "tanh": (EPI_TANH, 1.0)}
SPLITK_FLAGS = EPI_MASK | EPI_BIAS | EPI_ROWBIAS | EPI_RESID | EPI_RESID_INV | EPI_LRELU2


def _tile_case(tile, fname):
    BM, BN = TILES[tile]
    M, N = BM + 17, BN + 24                                # a whole tile, a whole fragment and one row; an N tail of three 8-column chunks
    flags, alpha = FLAG_SETS[fname]
    name = f"tile{tile}-{fname}"
    # conv1d k 3, dilation 2, Ci 24: K = 72 (a 64-chunk that spans taps and a partial one); images of 50 rows: boundaries inside fragments
    return Case(name, "tile-" + fname, lambda adt: conv1d_case(name, -(-M // 50), 50, 24, N, 3, 2, flags, alpha, tile, 8, M,
                                                                special_mask=True), tile, flags, M=M, N=N, K=72, ld_pad=8, HqWq=50)


def _cases():
    cs = [_tile_case(t, f) for t in sorted(TILES) for f in FLAG_SETS]
    # ---- direct epilogue: rows that are not 16-byte granular (N = ld = 12) or fp32 output
    cs.append(Case("direct-convpost", "direct", lambda adt: conv1d_case("direct-convpost", 3, 50, 32, 8, 7, 1, EPI_BIAS | EPI_F32OUT | EPI_TANH,
                                                                        ld_pad=0, kind="f32"), 0, EPI_BIAS | EPI_F32OUT | EPI_TANH, N=8, K=224))
    cs.append(Case("direct-f32-accum", "direct", lambda adt: conv1d_case("direct-f32-accum", 3, 50, 24, 12, 3, 2, EPI_F32OUT | EPI_ACCUM,
                                                                         ld_pad=0, kind="f32"), 0, EPI_F32OUT | EPI_ACCUM, N=12, K=72))
    FD = EPI_BIAS | EPI_ROWBIAS | EPI_MASK | EPI_RESID | EPI_RESID_INV | EPI_ACCUM | EPI_LRELU2
    for tile in (5, 12):
        nm = f"direct-16bit-tile{tile}"
        cs.append(Case(nm, "direct", lambda adt, nm=nm, tile=tile: conv1d_case(nm, 3, 50, 24, 12, 3, 2, FD, 0.5, tile, 0, 145, special_mask=True),
                       tile, FD, N=12, K=72, ld_pad=0, HqWq=50))
    # ---- M < 16 on a register-staged and on an LDS-DMA tile
    for tile in (6, 12):
        nm = f"m5-tile{tile}"
        cs.append(Case(nm, "mtail", lambda adt, nm=nm, tile=tile: gemm_nt_case(nm, 1, 1, 5, 72, 72, EPI_BIAS | EPI_RESID, tile), tile,
                       EPI_BIAS | EPI_RESID, M=5, N=72, K=72))
    # ---- Z > 1 on the LDS path: coff with a 16-bit output
    for tile in (6, 12):
        nm = f"batched-z4-tile{tile}"
        cs.append(Case(nm, "batched", lambda adt, nm=nm, tile=tile: gemm_nt_case(nm, 4, 2, 70, 136, 72, EPI_RESID, tile), tile, EPI_RESID,
                       Z=4, N=136, K=72))
    # ---- output row maps and strided gathers
    for s, k, p in ((4, 8, 2), (5, 11, 3)):
        nm = f"convT-s{s}k{k}"
        cs.append(Case(nm, "rowmap", lambda adt, nm=nm, s=s, k=k, p=p: convT1d_case(nm, 2, 37, 16, 24, k, s, p), 0, EPI_BIAS, osx=s, multi=True,
                       K=(k // s) * 16))
        cs.append(Case(nm + "-dgrad", "rowmap", lambda adt, nm=nm, s=s, k=k, p=p: convT1d_dgrad_case(nm + "-dgrad", 2, 37, 16, 24, k, s, p), 0, 0,
                       sx=s, K=k * 24))
    cs.append(Case("up2x-fwd", "rowmap", lambda adt: up2x_fwd_case("up2x-fwd", 2, 5, 7, 16, 24), 0, EPI_BIAS, osx=2, multi=True, K=64))
    cs.append(Case("up2x-bwd", "rowmap", lambda adt: up2x_bwd_case("up2x-bwd", 2, 5, 7, 16, 24), 0, 0, sx=2, K=384))
    cs.append(Case("conv2d-s2-pad01", "rowmap", lambda adt: conv2d_s2_case("conv2d-s2-pad01", 2, 9, 11, 16, 24), 0, EPI_BIAS, sx=2, K=144))
    # ---- GEGLU in the epilogue
    for tile in [3, 4, 5, 6] + DMA_TILES:
        BM, BN = TILES[tile]
        nm = f"geglu-tile{tile}"
        cs.append(Case(nm, "geglu", lambda adt, nm=nm, tile=tile, BM=BM, BN=BN: geglu_case(nm, BM + 17, 72, BN + 32, tile), tile,
                       EPI_GEGLU | EPI_BIAS, M=BM + 17, N=BN + 32, K=72))
    for tile in (3, 11, 14):
        nm = f"geglu-n96-tile{tile}"
        cs.append(Case(nm, "geglu", lambda adt, nm=nm, tile=tile: geglu_case(nm, 37, 72, 96, tile), tile, EPI_GEGLU | EPI_BIAS, M=37, N=96, K=72))
    for tile in LN_TILES:
        BM, BN = TILES[tile]
        nm = f"geglu-ln-tile{tile}"
        cs.append(Case(nm, "geglu-ln", lambda adt, nm=nm, tile=tile, BM=BM, BN=BN: geglu_case(nm, BM + 17, 72, BN + 32, tile, ln=True), tile,
                       EPI_GEGLU | EPI_BIAS | EPI_LNFOLD, M=BM + 17, N=BN + 32, K=72))
    for tile in (6, 12):
        nm = f"geglu-exact-gate-tile{tile}"
        cs.append(Case(nm, "geglu-exact", lambda adt, nm=nm, tile=tile: geglu_case(nm, 0, 16, 96, tile, exact_gate_adt=True, adt=adt), tile,
                       EPI_GEGLU, N=96, K=16, exact_gate=True))
    # ---- fused softmax backward (tile 1)
    cs.append(Case("softbwd", "softbwd", lambda adt: softbwd_case("softbwd", 2, 264, 72), 1, EPI_SOFTBWD, M=264, N=264, K=72))
    # ---- forced split-K plans against the unsplit tile 12 (deep K: structure, not sharpness)
    for fl, tag in ((SPLITK_FLAGS, ""), (SPLITK_FLAGS | EPI_NO_C, "-noc")):
        for plan in (12, 212, 313):
            nm = f"splitk{tag}-{plan}"
            cs.append(Case(nm, "splitk", lambda adt, nm="splitk" + tag, fl=fl, plan=plan: conv2d_3x3_case(nm, 4, 5, 5, 64, 72, fl, 0.5, plan),
                           plan, fl, M=100, N=72, K=576, HqWq=25, splitk=plan >= 100))
    # ---- the sign-bit tape of the vocoder on the generic tiles: mask factor from a bit (EPI_MASKBITS), sign bytes of the stored tensor
    # (EPI_BITS2) with and without the primary output; N = 8 / 16 sit inside one 32-column wave tile (the N-tail path of the mask), N = 88
    # spans tiles and leaves a tail.  Tile 0 = what the dispatcher picks, 6 = register-staged, 12 = LDS-DMA: every tile has its own
    # instantiation with the bit paths (csrc/gemm_conv.hip launch_cfg / launch_glds pick it by flag), so no forced tile lacks one.
    for fname, fl in BIT_FLAG_SETS.items():
        for N in (8, 16, 88):
            for tile in BIT_TILES:
                nm = f"bits-{fname}-n{N}-tile{tile}"
                cs.append(Case(nm, "bits", lambda adt, nm=nm, fl=fl, N=N, tile=tile: conv1d_case(nm, 2, 50, 24, N, 3, 2, fl, 1.0, tile, 8, 81,
                                                                                                  special_mask=True), tile, fl, M=81, N=N, K=72, HqWq=50))
    return cs


BIT_FLAG_SETS = {"maskbits-resid": EPI_MASKBITS | EPI_RESID, "lrelu2-bits2": EPI_LRELU2 | EPI_BITS2,
                 "lrelu2-bits2-noc": EPI_LRELU2 | EPI_BITS2 | EPI_NO_C}
BIT_TILES = (0, 6, 12)
CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def sharp_fraction(case, adt):
    """share of the written elements whose accumulation term exceeds the output term"""
    over = tot = 0
    for name, (val, bd, cnt) in case.expected(adt).items():
        w = cnt > 0
        ref = val[w].abs()
        kind = case.data(adt)[1][name].kind
        if kind == "f32":                                   # (4 u32 |ref| lies below A by construction: the condition speaks of 16-bit outputs)
            continue
        outt = 4 * U32 * ref if kind == "f32" else 1.5 * act_eps(adt) * ref + act_tiny(adt) / 2
        over += ((bd[w] - outt) > outt).sum().item()
        tot += int(w.sum())
    return over / max(tot, 1)


# ------------------------------------------------------------------------------------------------------------------ mutants
# name -> predicate: does the case exercise what the mutant breaks?
def _l0(case):
    return case.data(torch.float16)[0][0]


MUTANTS = {
    "drop_last_row": lambda c: c.family.startswith("tile-") or c.family in ("mtail", "geglu", "direct"),
    "drop_last_chunk": lambda c: c.family.startswith("tile-") or c.family in ("geglu", "geglu-ln", "batched"),
    "rowbias_neighbour": lambda c: bool(c.flags & EPI_ROWBIAS) and c.feat.get("HqWq", 16) % 16 != 0,
    "resid_no_inv": lambda c: bool(c.flags & EPI_RESID_INV),
    "alpha_after_accum": lambda c: bool(c.flags & EPI_ACCUM) and _l0(c).alpha != 1.0,
    "mask_zero_positive": lambda c: bool(c.flags & EPI_MASK),
    "skip_k_chunk": lambda c: not c.feat.get("exact_gate"),
    "oox_off_by_one": lambda c: "osx" in c.feat,
    "geglu_swap": lambda c: bool(c.flags & EPI_GEGLU),
    "geglu_bias_unpacked": lambda c: bool(c.flags & EPI_GEGLU) and bool(c.flags & EPI_BIAS),
    "geglu_erf_fp32": lambda c: bool(c.feat.get("exact_gate")),
    "mask_bit_reversed": lambda c: bool(c.flags & EPI_MASKBITS),
}
