"""Shared by tests/test_pair_bound_host.py (CPU) and tests/test_gpu_pair_elementwise.py (GPU): a float64 model of the fused
convolution pair (csrc/conv_pair.hip), its element-wise bound, an fp32 emulation, builders, the case table and mutants.

The model is written from the documented contract (csrc/conv_pair.h, the header comment of conv_pair.hip), not from the kernel body, and
rests on the single-launch model of tests/gemm_cases.py (G):
    1. stage `a` runs as a GemmDesc launch;
    2. its result h is the 16-bit tensor stage `b` reads as b.A (a.C2 under EPI_LRELU2, else a.C); outside [0, T) of each clip it is ZERO
       -- the zero padding of the second convolution, not the first stage evaluated there;
    3. stage `b` runs as a GemmDesc launch on it;
    4. of stage `a`, a.C2 reaches memory only when non-null, a.B2 under EPI_BITS2, a.C never.
PairDead: `skip` = output rows [skip0, skip1) of every clip, rounded INWARD to whole slabs of BMo rows (BMo = 256 - (lo + hi) of stage b for
a pair, 256 for a single stage), never all slabs: nothing of a skipped slab is written, neither b.C, b.C2, b.B2, a.C2, a.B2 nor the EPI_ACCUM
target.  `zero` = stage-a input rows [zero0, zero1) of every clip read as zeros, also where they are stage b's residual.

Both stages are evaluated on a time axis widened by HP rows on either side of every clip, so that "h outside the clip" is an explicit
array the model zeroes (and a mutant does not).

Bound, from the number formats only.  For stage a the kernel's 16-bit intermediate satisfies |h^ - h| <= beta_h, the single-launch bound
of G (accumulation term carried through the chain + output term), beta_h = 0 outside the clip.
    universal  |out - ref| <= P + A_b + output term against the reference built on the exact, unrounded h:
               P = sum_taps |w2| beta_h gathered like the convolution and carried through stage b's pointwise chain (mask factor <= 1,
               alpha, leaky-relu; not scaled by the residual), A_b the accumulation term with S built from |h| + beta_h;
    sharp      where the tape tensor a.C2 is stored: a.C2 against h within beta_h, then stage b against the model run ON THE STORED
               a.C2 BITS as its input with the plain single-launch bound (that input is a kernel output the first step verified;
               no tolerance is taken from it).
A sign byte of a bits-only intermediate is compared exactly outside the ambiguous set |h| <= A_a + tiny.
The C = 32, k = 3 cases (K = 96) are the sharp ones; the deep-K cases (up to K = 1408) are there for structure."""
import zlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from tests import gemm_cases as G
from tests.gemm_cases import (Buf, EPI_ACCUM, EPI_BIAS, EPI_BITS2, EPI_LRELU2, EPI_MASK, EPI_MASKBITS, EPI_NO_C, EPI_RESID, EPI_RESID_INV,
                              sentinel)

PAIR_ROWS = 256
HP = 50                                  # rows added on either side of every clip (the largest halo a stage may have)
SLOPE = 0.1


def halo(L):
    return max(0, max(-t for t in L.tdx)), max(0, max(L.tdx))


def slab_rows(a, b):
    lo, hi = halo(b)
    return PAIR_ROWS - lo - hi if a is not None else PAIR_ROWS


def skip_slabs(dead, T, BMo):
    """slabs [q0, q1) of every clip that `dead` skips: whole slabs inside [skip0, skip1) (the last, partial slab counts as inside when the
    interval reaches T), never all of them"""
    if dead is None or dead[1] <= dead[0]:
        return 0, 0
    nb = -(-T // BMo)
    lo = -(-max(dead[0], 0) // BMo)
    hi = nb if dead[1] >= T else dead[1] // BMo
    return (lo, hi) if hi > lo and hi - lo < nb else (0, 0)


def problem(a, b, dead=None):
    return SimpleNamespace(a=a, b=b, dead=dead)


def _copy(L, **kw):
    return SimpleNamespace(**{**vars(L), **kw})


def _widen(data, nclip, T, ld, fill=0.0):
    """(nclip * T, ld) flat -> (nclip * (T + 2 HP), ld) flat with HP rows of `fill` around every clip"""
    return F.pad(data.view(nclip, T, ld), (0, 0, HP, HP), value=fill).reshape(-1)


def _stage_a(p, st, adt, mut, emulate_order=None):
    """stage a on the widened axis -> (h, beta) as (nclip, T + 2 HP, C) with the rows outside the clip zeroed (unless the mutant computes
    them); emulate_order: return the fp32 emulation's 16-bit h^ instead of the exact h (beta = None)"""
    a, b = p.a, p.b
    T, C = b.Wq, b.N
    nclip, Tp = b.M // T, T + 2 * HP
    x = st[a.A].data.clone().view(nclip, T, C)
    if p.dead is not None and p.dead[3] > p.dead[2]:
        x[:, p.dead[2]:p.dead[3]] = 0.0
    xw = F.pad(x, (0, 0, HP, HP))
    if mut == "next_clip_row":                              # rows t >= T of a clip read on in memory (the next clip's row 0, ...) instead of zeros
        flat = x.reshape(-1, C)
        for c in range(nclip):
            idx = c * T + T + torch.arange(HP)
            idx = idx[idx < flat.shape[0]]
            xw[c, HP + T:HP + T + idx.numel()] = flat[idx]
    sx = {**st, "__ax": Buf("act", xw), "__hx": Buf("act", torch.zeros(nclip * Tp * C, dtype=torch.float64))}
    kw = dict(A="__ax", M=nclip * Tp, Wi=Tp, Wq=Tp, Wo=Tp, B2=None)
    loB = halo(b)[0]
    shift = loB if mut == "a_mask_at_output_row" else 0     # the mask of intermediate row i taken at row i + loB (the output row's)
    if a.flags & EPI_MASK:
        sx["__xx"] = Buf("act", torch.roll(_widen(st[a.X].data, nclip, T, a.ldx).view(-1, a.ldx), -shift, 0))
        kw["X"] = "__xx"
    if a.flags & EPI_MASKBITS:
        sx["__xb"] = Buf("bits", torch.roll(_widen(st[a.XB].data, nclip, T, a.ldxb).view(-1, a.ldxb), -shift, 0))
        kw["XB"] = "__xb"
    if a.flags & EPI_LRELU2:
        ax = _copy(a, flags=(a.flags | EPI_NO_C) & ~EPI_BITS2, C2="__hx", ldc2=C, **kw)
    else:
        ax = _copy(a, flags=a.flags & ~(EPI_NO_C | EPI_BITS2), C="__hx", ldc=C, **kw)
    inside = torch.zeros(nclip, Tp, 1, dtype=torch.bool)
    inside[:, HP:HP + T] = True
    if emulate_order is not None:
        ax.bias_first = C < 128 and not (a.flags & (EPI_MASK | EPI_MASKBITS))       # C = 128: the bias joins in the tail
        h = G.emulate([ax], sx, adt, emulate_order)["__hx"].view(nclip, Tp, C)
        return torch.where(inside, h, torch.zeros((), dtype=torch.float64)), None
    lm = mut if mut in ("mask_bit_reversed", "drop_last_tap") else None
    _, _, h, beta = G.run_launch(ax, sx, adt, lm)[-1]
    h, beta = h.view(nclip, Tp, C), beta.view(nclip, Tp, C)
    if mut != "h_outside_computed":
        h = torch.where(inside, h, torch.zeros((), dtype=torch.float64))
        beta = torch.where(inside, beta, torch.zeros((), dtype=torch.float64))
    return h, beta


def _stage_b_desc(p, mut):
    b = p.b
    tdx = [t + HP for t in b.tdx]
    if mut == "b_tap_shift":                                # the last tap of stage b reads one row further
        tdx[-1] += 1
    return _copy(b, A="__hx", Wi=b.Wq + 2 * HP, tdx=tdx)


def _resid_state(p, st, mut):
    """the buffers stage b sees beside its input: the zero rows also in the residual, the mutants of the slab residual"""
    a, b = p.a, p.b
    T, C = b.Wq, b.N
    out = dict(st)
    if (b.flags & EPI_RESID) and a is not None and b.R == a.A:
        r = st[b.R].data.clone().view(b.M // T, T, C)
        if p.dead is not None and p.dead[3] > p.dead[2] and mut != "zero_not_in_resid":
            r[:, p.dead[2]:p.dead[3]] = 0.0
        if mut == "resid_off_loA":                          # the slab row of output row r is r + loA + loB: here without the loA
            r = F.pad(r, (0, 0, halo(a)[0], 0))[:, :T]      # (the slab holds zeros before the clip)
        out[b.R] = Buf("act", r)
    return out


def _kept_rows(p, mut):
    """rows of the launch that are written: all but the skipped slabs"""
    a, b = p.a, p.b
    T = b.Wq
    BMo = slab_rows(a, b)
    q0, q1 = skip_slabs(p.dead, T, BMo)
    nb = -(-T // BMo)
    if q1 > q0:
        if mut == "skip_one_more":
            q0, q1 = (q0, q1 + 1) if q1 < nb else (q0 - 1, q1)
        if mut == "skip_one_fewer":
            q1 -= 1
    t = torch.arange(b.M) % T
    return ~((t >= q0 * BMo) & (t < q1 * BMo)), (q0, q1, BMo)


def run_pair(p, st, adt, mut=None, stored=None):
    """Float64 model of one pair launch (p.a None: a single stage).  -> list of writes (name, flat indices, values, bound, accumulates)
    as G.run_launch returns them; sign-bit writes carry (byte of ref > 0, byte of the free bits).
    stored: the flat float64 values of a.C2 as a kernel stored them -> the SHARP reference of stage b (plain bound)."""
    a, b = p.a, p.b
    T, C = b.Wq, b.N
    nclip = b.M // T
    keep, (q0, q1, BMo) = _kept_rows(p, mut)
    lm = mut if mut in ("mask_bit_reversed", "drop_last_tap") else None
    writes = []
    if a is None:
        wb = G.run_launch(_copy(b, tdx=b.tdx[:-1] + [b.tdx[-1] + 1]) if mut == "b_tap_shift" else b, st, adt, lm)
    else:
        h, beta = _stage_a(p, st, adt, mut)
        hin, bin_ = h[:, HP:HP + T].reshape(-1, C), beta[:, HP:HP + T].reshape(-1, C)
        m = torch.arange(b.M)
        if (a.flags & EPI_LRELU2) and a.C2 is not None:
            idx = m[:, None] * a.ldc2 + torch.arange(C)[None, :]
            writes.append((a.C2, idx[keep], hin[keep], bin_[keep], False))
            if mut == "halo_rows_written":                  # every slab stores the halo rows of its intermediate too
                lo, hi = halo(b)
                tt = m % T
                nb = -(-T // BMo)
                runs = [q for q in range(nb) if not q0 <= q < q1]
                extra = torch.zeros(b.M, dtype=torch.bool)
                for q in runs:
                    extra |= ((tt >= q * BMo - lo) & (tt < q * BMo)) | ((tt >= (q + 1) * BMo) & (tt < (q + 1) * BMo + hi))
                extra &= ~keep
                writes.append((a.C2, idx[extra], hin[extra], bin_[extra], False))
                zr = torch.cat([c * T + torch.arange(-lo, 0) for c in range(1, nclip)] + [c * T + T + torch.arange(hi) for c in range(nclip - 1)]
                               + [torch.zeros(0, dtype=torch.long)])
                zi = zr[:, None] * a.ldc2 + torch.arange(C)[None, :]
                writes.append((a.C2, zi, torch.zeros(zi.shape, dtype=torch.float64), torch.zeros(zi.shape, dtype=torch.float64), False))
        if a.flags & EPI_BITS2:
            eps, tiny = (G.act_eps(adt), G.act_tiny(adt)) if adt is not None else (0.0, 0.0)
            A_a = bin_ - 1.5 * eps * hin.abs() - tiny / 2   # the accumulation term of beta_h
            free = (hin.abs() <= A_a + tiny) if adt is not None else torch.zeros_like(hin, dtype=torch.bool)
            bidx = m[:, None] * a.ldb2 + torch.arange(C // 8)[None, :]
            writes.append((a.B2, bidx[keep], G.pack_bits(hin > 0)[keep], G.pack_bits(free)[keep], False))
        sb = _resid_state(p, st, mut)
        if stored is not None:
            sb["__hx"] = Buf("act", _widen(stored, nclip, T, C))
            wb = G.run_launch(_stage_b_desc(p, mut), sb, adt, lm)
        else:
            sb["__hx"] = Buf("act", h)
            wb = G.run_launch(_stage_b_desc(p, mut), sb, adt, lm, in_err={"__hx": beta.reshape(-1)})
    for name, idx, ref, bnd in wb:
        writes.append((name, idx[keep], ref[keep], bnd[keep], bool(b.flags & EPI_ACCUM) and name in (b.C, b.C2)))
    return writes


def _dead_as_launched(problems, mut):
    if mut != "group_wrong_dead":
        return problems
    order = sorted(range(len(problems)), key=lambda j: -(problems[j].a.K + problems[j].b.K))     # (stable, like the launcher's sort)
    return [problem(problems[j].a, problems[j].b, problems[i].dead) for i, j in enumerate(order)]


def expected_pair(problems, bufs, adt, mut=None, stored=None):
    """-> (outs, bits) like G.expected_all, for the problems of one (grouped or sequential) pair launch run in order.
    stored: {a.C2 name: flat values a kernel stored} -> the sharp reference (problems without an entry keep the universal one)."""
    state = {k: Buf(b.kind, b.data) for k, b in bufs.items()}
    outs = {}
    for p in _dead_as_launched(problems, mut):
        st = None
        if stored is not None and p.a is not None and p.a.C2 in stored:
            st = stored[p.a.C2]
        # an EPI_ACCUM launch onto what an EARLIER problem wrote inherits that problem's bound, in C and in C2 = leaky-relu of it (ldc = ldc2)
        prev = outs[p.b.C][1].clone() if p.b.C in outs else None
        for name, idx, ref, bnd, acc in run_pair(p, state, adt, mut, st):
            if name not in outs:
                nel = state[name].data.numel()
                outs[name] = (state[name].data, torch.zeros(nel, dtype=torch.float64), torch.zeros(nel, dtype=torch.int64))
            val, bd, cnt = outs[name]
            idx = idx.reshape(-1)
            ok = (idx >= 0) & (idx < val.numel())
            val[idx[ok]] = ref.reshape(-1)[ok]
            bd[idx[ok]] = bnd.reshape(-1)[ok] + (prev[idx[ok]] if acc and prev is not None else 0.0)
            cnt[idx[ok]] += 1
    return ({k: v for k, v in outs.items() if state[k].kind != "bits"}, {k: v for k, v in outs.items() if state[k].kind == "bits"})


def bits_source(problems):
    src = {}
    for p in problems:
        if p.a is not None and (p.a.flags & EPI_BITS2):
            src[p.a.B2] = (p.a.C2, p.a.ldc2, p.a.ldb2, p.b.N) if p.a.C2 is not None else None
        src.update(G.bits_source([p.b]))
    return src


def output_names(problems):
    names = []
    for p in problems:
        for L in (p.a, p.b):
            if L is not None:
                names += [n for n in (L.C, L.C2, L.B2) if n is not None]
    return list(dict.fromkeys(names))


def emulate_pair(problems, bufs, adt, order):
    """fp32 emulation of the kernel's arithmetic: bias-first accumulators at C < 128 without a mask, the bias in the tail at C = 128, the
    accumulation order, the intermediate rounded ONCE to 16 bits, the rest as G.emulate.  Skipped slabs keep what the buffers held.
    -> {name: flat float64 values}"""
    cur = {k: Buf(b.kind, b.data) for k, b in bufs.items()}
    for p in problems:
        a, b = p.a, p.b
        T, C = b.Wq, b.N
        nclip = b.M // T
        keep, _ = _kept_rows(p, None)
        new = {}
        if a is None:
            bb = _copy(b, bias_first=None if C < 128 else False)
            new = G.emulate([bb], cur, adt, order)
        else:
            h, _ = _stage_a(p, cur, adt, None, emulate_order=order)
            hin = h[:, HP:HP + T].reshape(-1, C)
            if (a.flags & EPI_LRELU2) and a.C2 is not None:
                new[a.C2] = hin.reshape(-1)
            if a.flags & EPI_BITS2:
                d = cur[a.B2].data.clone().view(b.M, a.ldb2)
                d[:, :C // 8] = G.pack_bits(hin > 0)
                new[a.B2] = d.reshape(-1)
            sb = _resid_state(p, cur, None)
            sb["__hx"] = Buf("act", h)
            bb = _copy(_stage_b_desc(p, None), bias_first=None if C < 128 else False)
            new.update(G.emulate([bb], sb, adt, order))
        for name, data in new.items():                      # rows of skipped slabs keep their contents
            ld = data.numel() // b.M
            old = cur[name].data.view(b.M, ld)
            cur[name] = Buf(cur[name].kind, torch.where(keep[:, None], data.view(b.M, ld), old))
    return {k: cur[k].data for k in output_names(problems)}


# ------------------------------------------------------------------------------------------------------------------ builders
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def conv_taps(k, dil, flip=False):
    pad = (k * dil - dil) // 2
    return [(pad - t * dil) if flip else (t * dil - pad) for t in range(k)]


def _special(g, x):
    """+0, -0 and subnormals of either sign in a quarter of the elements (a 16-bit mask source)"""
    tiny = G.act_tiny(torch.float16)
    sp = torch.tensor([0.0, -0.0, tiny, -tiny, 3 * tiny, -5 * tiny, 0.0, -0.0], dtype=torch.float64)
    flat = x.reshape(-1)
    pos = torch.randperm(flat.numel(), generator=g)[:flat.numel() // 4]
    flat[pos] = sp[torch.arange(pos.numel()) % 8]
    return x


def _stage(A, W, B, T, Cc, tdx, ldw, **kw):
    k = len(tdx)
    return G.launch(A=A, W=W, M=B * T, N=Cc, K=k * Cc, ldw=ldw, Hi=1, Wi=T, Ci=Cc, lda=Cc, Hq=1, Wq=T, ntaps=k, Ho=1, Wo=T, ldc=Cc, ldr=Cc,
                    ldx=Cc, ldc2=Cc, tdy=[0] * k, tdx=list(tdx), **kw)


def _pack(w, ldw, dgrad=False):
    C, k = w.shape[0], w.shape[2]
    wp = (w.permute(1, 2, 0) if dgrad else w.permute(0, 2, 1)).reshape(C, k * C)     # dgrad: [Cin][tap][Cout]
    return F.pad(wp, (0, ldw - k * C))


def forward_case(name, B, T, C, k, dil, tape="tensor", executor=False, sep_r=False, accum=False, ldw_pad=0, ldb2_pad=0, dead=None,
                 tdx_a=None, tdx_b=None, sfx=""):
    """a = conv(k, dil) BIAS | LRELU2 | NO_C -> b = conv(k, 1) BIAS | RESID | RESID_INV | LRELU2 with R = a.A.
    tape: 'tensor' (a.C2), 'bits' (a.B2 only, a.C2 null) or 'both'; executor: the vocoder executor's flag set."""
    g = _gen(name)
    tdx_a = conv_taps(k, dil) if tdx_a is None else tdx_a
    tdx_b = conv_taps(k, 1) if tdx_b is None else tdx_b
    ka, kb = len(tdx_a), len(tdx_b)
    x = torch.randn(B, T, C, generator=g).double()
    w1 = (torch.randn(C, C, ka, generator=g) / (C * ka) ** 0.5).double()
    w2 = (torch.randn(C, C, kb, generator=g) / (C * kb) ** 0.5).double()
    b1, b2 = 0.1 * torch.randn(C, generator=g).double(), 0.1 * torch.randn(C, generator=g).double()
    n = B * T * C
    X, W1, W2, H, HC, HB, Y, Y2, R2 = (s + sfx for s in ("X", "W1", "W2", "H", "HC", "HB", "Y", "Y2", "R2"))
    bufs = {X: Buf("act", x), W1: Buf("act", _pack(w1, ka * C + ldw_pad)), W2: Buf("act", _pack(w2, kb * C + ldw_pad)),
            "b1" + sfx: Buf("f32", b1), "b2" + sfx: Buf("f32", b2), HC: sentinel("act", n), Y: sentinel("act", n), Y2: sentinel("act", n)}
    fa = EPI_LRELU2 | EPI_NO_C | (0 if executor else EPI_BIAS)
    kwa = dict(C=HC, act_slope=SLOPE)
    if tape in ("tensor", "both"):
        bufs[H] = sentinel("act", n)
        kwa["C2"] = H
    if tape in ("bits", "both") or executor:
        ldb2 = C // 8 + ldb2_pad
        bufs[HB] = sentinel("bits", B * T * ldb2)
        kwa.update(B2=HB, ldb2=ldb2)
        fa |= EPI_BITS2
    if not executor:
        kwa["bias"] = "b1" + sfx
    a = _stage(X, W1, B, T, C, tdx_a, ka * C + ldw_pad, flags=fa, **kwa)
    fb = EPI_RESID | EPI_RESID_INV | EPI_LRELU2 | ((EPI_NO_C | EPI_ACCUM) if executor else EPI_BIAS) | (EPI_ACCUM if accum else 0)
    kwb = dict(C=Y, C2=Y2, R=X, resid_inv_slope=1.0 / SLOPE, act_slope=SLOPE)
    if not executor:
        kwb["bias"] = "b2" + sfx
    if sep_r:
        bufs[R2] = Buf("act", torch.randn(B, T, C, generator=g).double())
        kwb["R"] = R2
    if fb & EPI_ACCUM:
        bufs[Y] = Buf("act", torch.randn(n, generator=g).double())
    b = _stage(kwa.get("C2", HC), W2, B, T, C, tdx_b, kb * C + ldw_pad, flags=fb, **kwb)

    def torch_ref(bf):
        """conv1d -> leaky_relu -> conv1d + reconstructed residual (symmetric taps only) -> {name: (B T, C)}"""
        xx = bf[X].data.view(B, T, C).transpose(1, 2)
        h = F.leaky_relu(F.conv1d(xx, w1, None if executor else b1, padding=(k * dil - dil) // 2, dilation=dil), SLOPE)
        r = bf[kwb["R"]].data.view(B, T, C).transpose(1, 2)
        y = F.conv1d(h, w2, None if executor else b2, padding=(k - 1) // 2) + torch.where(r > 0, r, r / SLOPE)
        if fb & EPI_ACCUM:
            y = y + bf[Y].data.view(B, T, C).transpose(1, 2)
        out = {Y2: F.leaky_relu(y, SLOPE).transpose(1, 2).reshape(B * T, C)}
        if not (fb & EPI_NO_C):
            out[Y] = y.transpose(1, 2).reshape(B * T, C)
        if "C2" in kwa:
            out[H] = h.transpose(1, 2).reshape(B * T, C)
        return out
    return [problem(a, b, dead)], bufs, torch_ref


def backward_case(name, B, T, C, k, dil, maskbits=False, dead=None, sfx=""):
    """a = dgrad of conv(k, 1), flipped taps, MASK, a.C not written -> b = dgrad of conv(k, dil) MASK | RESID | ACCUM with R = a.A.
    maskbits: the same masks as sign-bit tensors (EPI_MASKBITS, ldxb = C / 8 + 4)."""
    g = _gen(name.replace("-maskbits", ""))                 # the MASKBITS twin has the operands of its MASK case
    gc = torch.randn(B, T, C, generator=g).double()
    ha = _special(g, torch.randn(B, T, C, generator=g).double())
    xa = _special(g, torch.randn(B, T, C, generator=g).double())
    prev = torch.randn(B, T, C, generator=g).double()
    w1 = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).double()
    w2 = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).double()
    n = B * T * C
    Gn, W1, W2, HA, XA, GH, DST, HAB, XAB = (s + sfx for s in ("G", "W1b", "W2b", "HA", "XA", "GH", "DST", "HAB", "XAB"))
    bufs = {Gn: Buf("act", gc), W1: Buf("act", _pack(w1, k * C, True)), W2: Buf("act", _pack(w2, k * C, True)), GH: sentinel("act", n),
            DST: Buf("act", prev)}
    if maskbits:
        ldxb = C // 8 + 4
        for nm, src in ((HAB, ha), (XAB, xa)):              # (the bits of the 16-bit mask sources: > 0 is the same question in fp16 and bf16 here)
            by = torch.randint(0, 256, (B * T, ldxb), generator=torch.Generator().manual_seed(7)).double()
            by[:, :C // 8] = G.pack_bits(src.view(B * T, C).to(torch.bfloat16).double() > 0)
            bufs[nm] = Buf("bits", by)
        ma = dict(flags=EPI_MASKBITS, XB=HAB, ldxb=ldxb)
        mb = dict(flags=EPI_MASKBITS | EPI_RESID | EPI_ACCUM, XB=XAB, ldxb=ldxb)
    else:
        bufs[HA], bufs[XA] = Buf("act", ha), Buf("act", xa)
        ma = dict(flags=EPI_MASK, X=HA)
        mb = dict(flags=EPI_MASK | EPI_RESID | EPI_ACCUM, X=XA)
    a = _stage(Gn, W2, B, T, C, conv_taps(k, 1, True), k * C, C=GH, mask_slope=SLOPE, **ma)
    b = _stage(GH, W1, B, T, C, conv_taps(k, dil, True), k * C, C=DST, R=Gn, mask_slope=SLOPE, **mb)

    def torch_ref(bf):
        """conv_transpose1d . mask -> conv_transpose1d . mask + residual + previous"""
        gcf = bf[Gn].data.view(B, T, C).transpose(1, 2)
        if maskbits:
            mh = G.unpack_bits(bf[HAB].data.view(B * T, -1)[:, :C // 8]).view(B, T, C)
            mx = G.unpack_bits(bf[XAB].data.view(B * T, -1)[:, :C // 8]).view(B, T, C)
        else:
            mh, mx = bf[HA].data.view(B, T, C) > 0, bf[XA].data.view(B, T, C) > 0
        g1 = F.conv_transpose1d(gcf, w2, padding=(k - 1) // 2) * torch.where(mh, 1.0, SLOPE).transpose(1, 2)
        g0 = F.conv_transpose1d(g1, w1, padding=(k * dil - dil) // 2, dilation=dil) * torch.where(mx, 1.0, SLOPE).transpose(1, 2) + gcf
        return {DST: (g0 + bf[DST].data.view(B, T, C).transpose(1, 2)).transpose(1, 2).reshape(B * T, C)}
    return [problem(a, b, dead)], bufs, torch_ref


def single_case(name, B, T, C, k, dil, flags):
    """a = NULL: one slab convolution, BIAS or BIAS | RESID | LRELU2 (the residual a separate tensor)"""
    g = _gen(name)
    x = torch.randn(B, T, C, generator=g).double()
    w = (torch.randn(C, C, k, generator=g) / (C * k) ** 0.5).double()
    bias = 0.1 * torch.randn(C, generator=g).double()
    n = B * T * C
    bufs = {"X": Buf("act", x), "W": Buf("act", _pack(w, k * C)), "bias": Buf("f32", bias), "Y": sentinel("act", n)}
    kw = dict(C="Y", bias="bias", flags=flags)
    if flags & EPI_RESID:
        bufs["R"] = Buf("act", torch.randn(n, generator=g).double())
        kw["R"] = "R"
    if flags & EPI_LRELU2:
        bufs["Y2"] = sentinel("act", n)
        kw.update(C2="Y2", act_slope=SLOPE)
    b = _stage("X", "W", B, T, C, conv_taps(k, dil), k * C, **kw)

    def torch_ref(bf):
        y = F.conv1d(bf["X"].data.view(B, T, C).transpose(1, 2), w, bias, padding=(k * dil - dil) // 2, dilation=dil).transpose(1, 2).reshape(B * T, C)
        if flags & EPI_RESID:
            y = y + bf["R"].data.view(B * T, C)
        out = {"Y": y}
        if flags & EPI_LRELU2:
            out["Y2"] = F.leaky_relu(y, SLOPE)
        return out
    return [problem(None, b)], bufs, torch_ref


def group_case(name, C, ks, shapes, dil=3, same_c=False, deads=None, backward=False):
    """the branches of one resblock step as one grouped launch: forward pairs of kernel sizes ks, (B, T) per problem.
    same_c: every problem accumulates into the first one's C (the launcher then runs them one after the other)."""
    problems, bufs = [], {}
    for j, (k, (B, T)) in enumerate(zip(ks, shapes)):
        dead = deads[j] if deads else None
        if backward:
            ps, bf, _ = backward_case(f"{name}-{j}", B, T, C, k, dil, dead=dead, sfx=str(j))
        else:
            ps, bf, _ = forward_case(f"{name}-{j}", B, T, C, k, dil, accum=same_c, dead=dead, sfx=str(j))
        bufs.update(bf)
        if same_c and j > 0:
            del bufs[ps[0].b.C]
            ps[0].b.C = problems[0].b.C
        problems += ps
    return problems, bufs, None


# ------------------------------------------------------------------------------------------------------------------ case table
class PairCase:
    """name, family, builder, how it is launched ('pair', 'group', 'dead', 'group_dead') and its features"""

    def __init__(self, name, family, build, how="pair", **feat):
        self.name, self.family, self._build, self.how, self.feat = name, family, build, how, feat
        self._cache = {}

    def data(self, adt):
        if adt not in self._cache:
            problems, bufs, tref = self._build()
            self._cache[adt] = (problems, {k: b.rounded(adt) for k, b in bufs.items()}, tref)
        return self._cache[adt]

    def expected(self, adt, mut=None):
        key = ("exp", adt, mut)
        if key not in self._cache:
            problems, bufs, _ = self.data(adt)
            self._cache[key] = expected_pair(problems, bufs, adt, mut)
        return self._cache[key]


GRID = [(3, 1), (7, 3), (11, 5)]
WIDTHS = (32, 64, 128)
SKIP_SPANS = {                                                       # name -> (span as a function of BMo and T, slabs skipped of 4)
    "slab1": (lambda m, T: (m - 3, 2 * m + 9), 1), "slab0": (lambda m, T: (0, m + 1), 1), "slab2-and-last": (lambda m, T: (2 * m, T), 2),
    "inside-slab0": (lambda m, T: (10, m - 1), 0), "whole-clip": (lambda m, T: (0, T), 0)}


def fwd_bmo(k):
    return PAIR_ROWS - (k - 1)


def bwd_bmo(k, dil):
    return PAIR_ROWS - (k - 1) * dil


def _cases():
    cs = []

    def add(name, family, build, how="pair", **feat):
        cs.append(PairCase(name, family, build, how, **feat))

    # ---- forward grid: three slabs, a last slab of 3 rows, a clip boundary inside a halo
    for C in WIDTHS:
        for k, dil in GRID:
            nm, T = f"fwd-c{C}-k{k}d{dil}", 2 * fwd_bmo(k) + 3
            add(nm, "fwd", lambda nm=nm, T=T, C=C, k=k, dil=dil: forward_case(nm, 2, T, C, k, dil), C=C, k=k, dil=dil, T=T, sharp=True)
    # ---- forward variants, one shape per width
    for C, (k, dil) in zip(WIDTHS, GRID):
        T = 2 * fwd_bmo(k) + 3
        variants = {"tape-bits": dict(tape="bits"), "tape-both": dict(tape="both"), "executor": dict(executor=True),
                    "sep-r": dict(sep_r=True), "accum": dict(accum=True), "ldw": dict(ldw_pad=8), "ldb2": dict(tape="both", ldb2_pad=3)}
        for v, kw in variants.items():
            nm = f"fwd-{v}-c{C}-k{k}d{dil}"
            add(nm, "fwd-variant", lambda nm=nm, T=T, C=C, k=k, dil=dil, kw=kw: forward_case(nm, 2, T, C, k, dil, **kw), C=C, k=k, dil=dil, T=T,
                variant=v, sharp=kw.get("tape", "tensor") != "bits" and not kw.get("executor"), bits_only=kw.get("tape") == "bits" or bool(kw.get("executor")))
    # ---- T edges
    for C, k, dil, B, Ts in ((64, 7, 3, 3, (1, 5, 249, 250, 251)), (32, 3, 1, 2, (254, 255)), (128, 11, 5, 2, (246, 247))):
        for T in Ts:
            nm = f"fwd-edge-c{C}-k{k}d{dil}-t{T}"
            add(nm, "fwd-edge", lambda nm=nm, T=T, C=C, k=k, dil=dil, B=B: forward_case(nm, B, T, C, k, dil), C=C, k=k, dil=dil, T=T, sharp=True)
    # ---- backward grid and its MASKBITS twins
    for C in WIDTHS:
        for k, dil in GRID:
            T = 2 * bwd_bmo(k, dil) + 3
            for mbits in (False, True):
                nm = f"bwd-c{C}-k{k}d{dil}" + ("-maskbits" if mbits else "")
                add(nm, "bwd", lambda nm=nm, T=T, C=C, k=k, dil=dil, mbits=mbits: backward_case(nm, 2, T, C, k, dil, maskbits=mbits), C=C, k=k,
                    dil=dil, T=T, maskbits=mbits)
    # ---- single stage
    for C in WIDTHS:
        for T in (255, 256, 257):
            for fname, fl in (("bias", EPI_BIAS), ("bias-resid-lrelu2", EPI_BIAS | EPI_RESID | EPI_LRELU2)):
                nm = f"single-c{C}-t{T}-{fname}"
                add(nm, "single", lambda nm=nm, T=T, C=C, fl=fl: single_case(nm, 2, T, C, 7, 3, fl), C=C, k=7, dil=3, T=T)
    # ---- tap shapes the eligibility test accepts but the vocoder never uses (both stages with the same taps)
    taps = {"k1": [0], "k2": [0, 1], "causal-k3d2": [-4, -2, 0], "k16d3": [t * 3 - 22 for t in range(16)]}
    for C in (32, 64):
        for tn, tdx in taps.items():
            lo, hi = max(0, -min(tdx)), max(0, max(tdx))
            nm, T = f"taps-{tn}-c{C}", 2 * (PAIR_ROWS - lo - hi) + 3
            add(nm, "taps", lambda nm=nm, T=T, C=C, tdx=tdx: forward_case(nm, 2, T, C, len(tdx), 1, tdx_a=tdx, tdx_b=tdx), C=C, k=len(tdx), T=T,
                sharp=True)
    # ---- grouped launches: the sort permutes (k = 3, 11, 7), another (B, T) per problem
    shapes = [(2, 300), (1, 520), (3, 100)]
    for C in WIDTHS:
        add(f"group3-c{C}", "group", lambda C=C: group_case(f"group3-c{C}", C, (3, 11, 7), shapes), "group", C=C)
        add(f"group2-c{C}", "group", lambda C=C: group_case(f"group2-c{C}", C, (3, 11), shapes[:2]), "group", C=C)
        add(f"group-same-c-c{C}", "group", lambda C=C: group_case(f"group-same-c-c{C}", C, (3, 7), [(2, 300), (2, 300)], same_c=True), "group",
            C=C, sequential=True)
    # ---- dead rows: four slabs (the last of 5 rows)
    for C, spans in ((64, list(SKIP_SPANS)), (32, ["slab1"]), (128, ["slab1"])):
        k, dil = 7, 3
        for sp in spans:
            fn, nskip = SKIP_SPANS[sp]
            m, T = fwd_bmo(k), 3 * fwd_bmo(k) + 5
            nm = f"dead-fwd-c{C}-{sp}"
            add(nm, "dead", lambda nm=nm, T=T, C=C, d=fn(m, T) + (0, 0): forward_case(nm, 2, T, C, k, dil, tape="both", dead=d), "dead", C=C, k=k,
                dil=dil, T=T, skipped=nskip, total=4, sharp=False)
            m, T = bwd_bmo(k, dil), 3 * bwd_bmo(k, dil) + 5
            nm = f"dead-bwd-c{C}-{sp}"
            add(nm, "dead", lambda nm=nm, T=T, C=C, d=fn(m, T) + (m - 7, m + 40): backward_case(nm, 2, T, C, k, dil, dead=d), "dead", C=C, k=k,
                dil=dil, T=T, skipped=nskip, total=4, zero=(m - 7, m + 40), nan_rows="G")
    gd = [(250 - 3, 2 * 250 + 9, 0, 0), (0, 0, 0, 0), (0, 255, 0, 0)]          # k = 7: BMo = 250, slab 1; k = 11: no span; k = 3: BMo = 254, slab 0
    add("dead-group-c64", "dead", lambda: group_case("dead-group-c64", 64, (7, 11, 3), [(2, 755), (1, 520), (2, 600)], deads=gd), "group_dead",
        C=64, grouped=True)
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def sharp_fraction(outs, bufs, adt):
    """share of the written 16-bit elements whose bound beyond the output term exceeds the output term"""
    over = tot = 0
    for name, (val, bd, cnt) in outs.items():
        w = cnt > 0
        outt = 1.5 * G.act_eps(adt) * val[w].abs() + G.act_tiny(adt) / 2
        over += ((bd[w] - outt) > outt).sum().item()
        tot += int(w.sum())
    return over / max(tot, 1)


# ------------------------------------------------------------------------------------------------------------------ mutants
def _p0(c):
    return c.data(torch.float16)[0][0]


def _has_a(c):
    return _p0(c).a is not None


MUTANTS = {
    # h outside the clip computed instead of zero: shows wherever stage b reaches outside (every pair with a stage-b halo)
    # (backward the out-of-clip rows carry the mask slope 0.1: at K = 1408 that stays inside the universal bound of a bf16 build -- ratio
    # 0.82 from the reference alone --, so the deepest backward shape is left to its forward twin)
    "h_outside_computed": lambda c: _has_a(c) and sum(halo(_p0(c).b)) > 0 and not (c.family == "bwd" and _p0(c).b.K > 1024),
    "b_tap_shift": lambda c: _p0(c).b.Wq > abs(_p0(c).b.tdx[-1]) + 1,         # (a clip shorter than the tap's reach reads zeros either way)
    "resid_off_loA": lambda c: _has_a(c) and _p0(c).b.R == _p0(c).a.A and halo(_p0(c).a)[0] > 0,
    # (with the last slabs of every clip skipped, no written row reads past the end of a clip that has a successor;
    # and the smallest forward tap of stage a must land on a row that exists: <= the rows that follow the first clip)
    "next_clip_row": lambda c: _has_a(c) and halo(_p0(c).a)[1] > 0 and "and-last" not in c.name
    and min(t for t in _p0(c).a.tdx if t > 0) <= _p0(c).b.M - _p0(c).b.Wq,
    "a_mask_at_output_row": lambda c: _has_a(c) and bool(_p0(c).a.flags & (EPI_MASK | EPI_MASKBITS)) and halo(_p0(c).b)[0] > 0,
    "mask_bit_reversed": lambda c: _has_a(c) and bool(_p0(c).a.flags & EPI_MASKBITS),
    "drop_last_tap": lambda c: c.feat.get("C") == 32 and _p0(c).b.ntaps % 2 == 1 and _p0(c).b.ntaps > 1,
    "halo_rows_written": lambda c: _has_a(c) and _p0(c).a.C2 is not None and sum(halo(_p0(c).b)) > 0 and _p0(c).b.M > _p0(c).b.Wq,
    "skip_one_more": lambda c: c.feat.get("skipped", 0) > 0,
    "skip_one_fewer": lambda c: c.feat.get("skipped", 0) > 0,
    "zero_not_in_resid": lambda c: "zero" in c.feat,
    "group_wrong_dead": lambda c: bool(c.feat.get("grouped")),
}
