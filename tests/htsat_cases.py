"""Shared by tests/test_htsat_bound_host.py (CPU) and tests/test_gpu_htsat_elementwise.py (GPU): float64 models of the ten kernels of the
CLAP HTS-AT tower (csrc/htsat.hip), their element-wise error bounds, fp32 emulations of the documented arithmetic, the case tables and
mutants of the models.

The models are written from the network's definition (transformers ClapAudioModel; tests/test_htsat_bound_host.py checks them against its
modules in float64), not from the kernels, and are structurally different from them:
    LayerNorm rows   plain rows, or the rows of a patch merging: the strided slices [0::2, 0::2] | [1::2, 0::2] | [0::2, 1::2] | [1::2, 1::2]
                     of the (B, H, W, C) grid, concatenated along the channels
    GELU             u Phi(u) with Phi = erfc(-u / sqrt 2) / 2 (no 1 + erf cancellation in the reference)
    window attention torch.roll(-shift), windows by reshape / permute, the mask from an image of region labels over the slices
                     (0, -8), (-8, -shift), (-shift, None) with -100 where labels differ, the relative position index from coordinate
                     differences (Swin), softmax in float64, the partition reversed, rolled back
    embed            BatchNorm (eval) per mel bin -> bicubic stretch of the time axis -> fold img[c bins + f][tt] = X[c T + tt][f] ->
                     conv2d(4 x 4, stride 4) -> LayerNorm.  Bicubic taps by torch's rule: source index float32(frames - 1) /
                     float32(Tout - 1) * float32(t) IN FLOAT32, A = -0.75, indices clamped at the borders, identity when frames == Tout
    Gram             G = F^T F / T
Every backward reference is torch.autograd on the float64 forward model (`dimg`, the gradient at the stretched image, is the gradient
of a zero tensor added there).  Inputs are rounded to the activation type or to fp32 first, exactly as a kernel sees them.

Bounds (from the number formats and operation counts only, never from a kernel's output).  u32 = 2^-24, ulp = 2 u32 (an fp32 ulp is at
most that, relative), eps_a = unit roundoff and tiny = smallest subnormal of the activation type.  A 16-bit output carries one rounding,
eps_a |ref| + tiny / 2, plus an fp32 term; an fp32 output the fp32 term only.  The fp32 term is c u32 S with S the sum of absolute terms
carried through the chain and c the number of fp32 operations on the path (first order), per kernel:
  device functions (ASSUMPTIONS: nobody has measured them here, and the HIP math API tables are not shipped with this toolchain):
    rsqrtf within RSQRT_ULP = 2 ulp (what tests/gemm_cases.py assumes), erff within ERF_ULP = 4 ulp, __expf within EXP_ULP = 2 ulp of
    exp2 of ITS argument -- it multiplies by log2 e first, so a relative error |x| u32 comes on top (2 |x| u32 with the rounded constant);
    at the -100 mask that is 200 u32.
  LayerNorm rows (two-pass; a thread adds the 8 ceil(nch / tpr) values of its chunks, then log2 tpr shuffle steps: chain d):
    d_mean = (d + 1) u32 mean|x|,   d_var = (d + 6) u32 var + d_mean^2   (sum (x - m')^2 / n = var + (m' - mean)^2: the offset survives)
    d_rstd = the larger one-sided change of 1 / sqrt(v + eps) over var +- d_var, + RSQRT_ULP ulp rstd          (valid at var = 0)
    e_xh   = rstd d_mean + |x - mean| d_rstd + d_mean d_rstd + 2 u32 |xhat|
    y      : |gamma| e_xh + 2 u32 (|xhat gamma| + |beta|)                                         c = 4 beside the statistics
    dx     : g = dy gamma (1 rounding), mg = sum g / n (d + 1), mgx = sum g xhat / n (d + 2, carrying e_xh), t = g - mg - xhat mgx (3),
             dx = rstd t + add: rstd e_t + |t| d_rstd + 2 u32 |rstd t| + u32 (|add| + |ref|)
  GELU  z = u / sqrt 2 (constant and product: 1.5 u32 |z| erf'(z)), erff (ERF_ULP ulp |erf|), 1 + erf (u32 |1 + erf|): A1; 0.5 u (.): 2 u32.
        For negative u the sum 1 + erf cancels: the ABSOLUTE term 0.5 |u| ERF_ULP ulp remains (at u = -4 about one fp16 ulp of the
        result).  transformers' own GELU has the same cancellation: documented behaviour that is bounded, not a bug.
        y  : 0.5 |u| A1 + 2 u32 |ref|
        du : gelu' = Phi + u phi, phi = exp(-u^2 / 2) / sqrt(2 pi): |dy| (0.5 A1 + |u phi| ((4 u^2 / 2 + 3) u32 + EXP_ULP ulp) + u32 |gelu'|)
             + u32 |ref|                                   (the exponent's two roundings and __expf's two: 4 |arg| u32)
  window attention (one lane per query; a score is 24 FMAs onto the bias, in channel order):
        score  d_s = u32 (sum_k |bias + sum_{d <= k} scale q_d k_d| + 2 scale sum_d |q_d k_d|) + u32 |s| where the -100 is added
               (every FMA rounds its partial sum once; the scaled q carries two roundings.  The worst case 26 u32 (scale sum |q k| +
               |bias|) is four times that for unit-normal q and k, and with it a fifth of the outputs could not be sharp)
        e_j = __expf(s_j - max): relative delta_j = d_s_j + u32 |a_j| + EXP_ULP ulp + 2 |a_j| u32,  a_j = s_j - max; the error of the
        maximum itself is common to the row and cancels in e_j / sum e
        Every longer sum is bounded the same way, chain(t) = u32 sum_k |sum_{j <= k} t_j| in the kernel's order (keys, queries and
        channels ascending): at most n u32 sum |t|, and that only when nothing cancels.
        o_d = (sum_j e_j v_jd) / sum_j e_j:  sum_j p_j |v_jd| (delta_j + Delta) + (chain(p) + 3 u32) sum_j p_j |v_jd| + chain(p v_d),
        Delta = sum_k p_k delta_k    (the count: 2 x 24 + 2 for a score pair, 64 for the row sum, 64 for the P V sum, 3 for 1 / sum and
        the products)
        (chain(p), the row sum of e: a step is also never off by more than what it adds, min(u32 partial sum, p_k))
        backward  p'_j = p_j (1 + eps_j - sum_k p_k eps_k) (1 + c_j) with |eps_j| <= delta_j (the exponentials) and |c_j| <= kap = chain(p) +
        3 u32 (row sum, 1 / sum, product).  The eps part keeps sum_j p_j = 1: in delta = sum_j p_j dP_j it leaves sum_j eps_j dS_j, bounded
        by sum_j delta_j |dS_j|, not sum_j p_j delta_j |dP_j| -- a near one-hot row, where dS is small beside p dP, keeps its
        resolution.  p_j: p_j (delta_j + Delta - 2 p_j delta_j + kap);  dP = dO . v: chain over 24;  delta: sum_j delta_j |dS_j| + kap sum_j
        p_j |dP_j| + sum_j p_j e_dP_j + chain over 64;  dS = p (dP - delta): |dS_j| (delta_j + Delta + kap) + p_j (e_dP_j + e_delta), 2 more;  dq = scale sum_j dS k, dk = sum_i dS (scale q): chain over 64, + 2 each;  dv = sum_i p dO: chain
        over 64    (2 x 64 + 2 x 24 + 16 operations on the longest path)
  embed (one thread per token, every sum sequential):
        pixel  a (sum_k w_k mel_k) + c with a = w / sqrt(var + eps) and c = b - m a folded on the host: 7 u32 |a| sum |w mel| (a term of the
               stretch: the table weight's rounding, its product, at most 3 sums; a's own rounding; the product with a) + u32 (|b| +
               3 |m a|) (c: a's rounding, m a, the difference) + u32 |pix|
        conv   sum_k |W| d_pix + 17 u32 (sum |W pix| + |bias|);   LayerNorm over E as above with d = E and the conv error carried in
        dimg   LayerNorm backward as above with d = E, dp_q = sum_n W_nq dpre_n (E FMAs), x a: 2 u32
        dmel   sum over the n_k taps that read frame k: sum |w| e_dimg + (n_k + 3) u32 sum |w dimg|, x scale: u32 |ref|
  Gram  G: (T + 2) u32 |F|^T |F| / T (T FMAs, 1 / T and the product AFTER the sum);  dF: (C + 3) u32 |F| (|dG| + |dG|^T) / T
The GPU tests print the observed err / bound per case; the largest per kernel is recorded in profiles/htsat_elementwise.txt.

Sharpness.  A bound whose fp32 term swamps the output rounding cannot see a wrong rounding or a slightly wrong weight.
sharp_fraction() is the share of elements whose fp32 term exceeds eps_a |ref|; tests/test_htsat_bound_host.py caps it at 10 % for the
16-bit forward outputs and at 30 % for the 16-bit backward outputs.  Exempt, each for its stated reason: the GELU case of special values
only (half of them sit in the cancellation range on purpose, and a reference of exactly 0 counts as unsharp by definition) and the
LayerNorm rows whose variance is zero or a rounding (eps decides; the output is beta plus rounding noise times 1 / sqrt eps).  Every
attention case is capped, the peaked one included.  fp32 outputs have no rounding term; their median bound / |ref| is reported.

Emulation share, as in tests/gemm_cases.py: err <= bound / 2 for fp32 outputs; for 16-bit outputs
err <= (eps_a |ref| + tiny / 2) + (bound - eps_a |ref| - tiny / 2) / 2."""
import math
import zlib
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from tests.gemm_cases import U32, SENT16, SENT32, act_eps, act_tiny  # noqa: F401  (the sentinels are re-exported to the GPU test)

WS, WT, HD = 8, 64, 24
RSQRT_ULP, ERF_ULP, EXP_ULP = 2.0, 4.0, 2.0
ULP = 2 * U32
UF32 = 2.0 ** -149
SQRT2 = math.sqrt(2.0)
LN_MAX_WIDTH = 1536
EMB_MAX = 128


def cdiv(a, b):
    return -(-a // b)


def rd(t, adt):
    """values of the activation type (or of fp32: adt None) as float64"""
    return (t.float() if adt is None else t.to(adt)).double()


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def rounding(ref, adt):
    return act_eps(adt) * ref.abs() + act_tiny(adt) / 2


def sharp_fraction(bound, ref, adt):
    """share of the elements whose fp32 term exceeds eps_a |ref|"""
    return ((bound - rounding(ref, adt)) > act_eps(adt) * ref.abs()).double().mean().item()


def emu_limit(bound, ref=None, adt=None):
    if adt is None:
        return bound / 2
    r = rounding(ref, adt)
    return r + (bound - r) / 2


def out_bound(fp32_term, ref, adt):
    """adt None: an fp32 output"""
    return fp32_term if adt is None else rounding(ref, adt) + fp32_term


def _rstd_err(var, d_var, eps):
    rstd = 1.0 / torch.sqrt(var + eps)
    lo = 1.0 / torch.sqrt(var + d_var + eps)
    hi = 1.0 / torch.sqrt((var - d_var).clamp_min(0.0) + eps)
    return torch.maximum(rstd - lo, hi - rstd) + RSQRT_ULP * ULP * rstd


# ===================================================================================================================== LayerNorm rows
def ln_geom(Cw):
    """(threads per row, rows per workgroup, 8-channel chunks) as csrc/htsat.hip documents them: a power of two of threads, at most 64"""
    nch, tpr = Cw // 8, 1
    while tpr < nch and tpr < 64:
        tpr *= 2
    return tpr, 256 // tpr, nch


def ln_chain(Cw):
    tpr, _, nch = ln_geom(Cw)
    return 8 * cdiv(nch, tpr) + int(math.log2(tpr))


def merge_rows(x, mut=None):
    """(B, H, W, C) -> (B, H / 2, W / 2, 4 C), the rows of a patch merging"""
    a, b, c, d = x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]
    if mut == "merge_order":
        b, c = c, b                                                   # (0,0) (0,1) (1,0) (1,1)
    return torch.cat([a, b, c, d], -1)


def ln_gather(x, C, merge, H, W, rows, mut=None):
    """x: flat, the kernel's token-major layout -> (rows, row width)"""
    if not merge:
        return x.view(-1, C)[:rows]
    if mut == "swap_hw":
        H, W = W, H
    return merge_rows(x.view(-1, H, W, C), mut).reshape(-1, 4 * C)[:rows]


def ln_forward(xr, gamma, beta, eps, mut=None):
    n = xr.shape[1]
    mean = xr.mean(1, keepdim=True)
    var = ((xr - mean) ** 2).sum(1, keepdim=True) / (n - 1 if mut == "unbiased" else n)
    rstd = 1.0 / (var.sqrt() + eps) if mut == "eps_outside" else 1.0 / torch.sqrt(var + eps)
    return (xr - mean) * rstd * gamma + beta


def _ln_stats(xr, eps, d, e_x=None):
    """statistics of rows and their fp32 errors; e_x: error the row's values already carry (the embed's convolution)"""
    mean = xr.mean(1, keepdim=True)
    xc = xr - mean
    var = (xc * xc).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    d_mean = (d + 1) * U32 * xr.abs().mean(1, keepdim=True)
    if e_x is None:
        ec = d_mean
        d_var = (d + 6) * U32 * var + d_mean ** 2 + 2 * UF32
    else:
        d_mean = d_mean + e_x.mean(1, keepdim=True)
        ec = e_x + d_mean
        m2 = (ec * ec).mean(1, keepdim=True)
        d_var = (d + 6) * U32 * var + 2 * torch.sqrt(var * m2) + m2 + 2 * UF32
    d_rstd = _rstd_err(var, d_var, eps)
    xh = xc * rstd
    e_xh = rstd * ec + xc.abs() * d_rstd + ec * d_rstd + 2 * U32 * xh.abs()
    return NS(mean=mean, var=var, rstd=rstd, xh=xh, d_rstd=d_rstd, e_xh=e_xh)


def ln_forward_term(xr, gamma, beta, eps, d, e_x=None):
    s = _ln_stats(xr, eps, d, e_x)
    return gamma.abs() * s.e_xh + 2 * U32 * ((s.xh * gamma).abs() + beta.abs()) + 2 * UF32


def ln_backward_term(xr, dy, gamma, eps, d, e_x=None):
    """-> (fp32 term of rstd (g - mean g - xhat mean(g xhat)), that value) in the rows' layout; without `add`"""
    s = _ln_stats(xr, eps, d, e_x)
    n = xr.shape[1]
    g = dy * gamma
    e_g = U32 * g.abs()
    mg, mgx = g.mean(1, keepdim=True), (g * s.xh).mean(1, keepdim=True)
    d_mg = (e_g.sum(1, keepdim=True) + (d + 1) * U32 * g.abs().sum(1, keepdim=True)) / n
    d_mgx = ((e_g * s.xh.abs() + g.abs() * s.e_xh).sum(1, keepdim=True) + (d + 2) * U32 * (g * s.xh).abs().sum(1, keepdim=True)) / n
    t = g - mg - s.xh * mgx
    e_t = e_g + d_mg + s.xh.abs() * d_mgx + mgx.abs() * s.e_xh + s.e_xh * d_mgx + 3 * U32 * (g.abs() + mg.abs() + (s.xh * mgx).abs())
    val = s.rstd * t
    return s.rstd * e_t + t.abs() * s.d_rstd + e_t * s.d_rstd + 2 * U32 * val.abs() + 4 * UF32, val


def ln_backward(x, dy, add, gamma, C, merge, H, W, rows, eps, mut=None):
    """autograd of <dy, LayerNorm(rows of x)> at x (+ add) -> flat, x's layout.  Tokens no row reads get 0 (the kernel leaves them alone)."""
    xg = x.clone().requires_grad_(True)
    y = ln_forward(ln_gather(xg, C, merge, H, W, rows, mut), gamma, torch.zeros_like(gamma), eps, mut)
    (gr,) = torch.autograd.grad((y * dy).sum(), xg)
    if add is not None and mut != "drop_add":
        gr = gr + add
    return gr


def ln_source_index(n, C, merge, H, W, rows):
    """flat index in x of every element of the rows, in the rows' layout (every source element at most once)"""
    return ln_gather(torch.arange(n, dtype=torch.float64), C, merge, H, W, rows).long()


def ln_emulate_forward(xr, gamma, beta, eps, adt):
    x, n = xr.float(), xr.shape[1]
    mean = x.sum(1, keepdim=True, dtype=torch.float32) / n
    dd = x - mean
    rstd = torch.rsqrt((dd * dd).sum(1, keepdim=True, dtype=torch.float32) / n + torch.tensor(eps, dtype=torch.float32))
    return rd(dd * rstd * gamma.float() + beta.float(), adt)


def ln_emulate_backward(xr, dy, addr, gamma, eps, adt):
    """rows' layout in, rows' layout out (addr: `add` gathered like x, or None)"""
    x, n = xr.float(), xr.shape[1]
    mean = x.sum(1, keepdim=True, dtype=torch.float32) / n
    dd = x - mean
    rstd = torch.rsqrt((dd * dd).sum(1, keepdim=True, dtype=torch.float32) / n + torch.tensor(eps, dtype=torch.float32))
    xh = dd * rstd
    g = dy.float() * gamma.float()
    mg, mgx = g.sum(1, keepdim=True, dtype=torch.float32) / n, (g * xh).sum(1, keepdim=True, dtype=torch.float32) / n
    o = rstd * (g - mg - xh * mgx)
    if addr is not None:
        o = o + addr.float()
    return rd(o, adt)


class LnCase:
    def __init__(self, name, C, rows, merge=0, H=1, W=1, family="plain", out32=False, eps=1e-5):
        self.name, self.C, self.rows, self.merge, self.H, self.W, self.family, self.out32, self.eps = name, C, rows, merge, H, W, family, out32, eps
        self.Cw = 4 * C if merge else C
        self.d = ln_chain(self.Cw)
        self.tokens = cdiv(rows, (H // 2) * (W // 2)) * H * W if merge else rows
        self.exempt_rows = [0, 1] if family == "const" else []           # variance zero / a rounding: eps decides (module docstring)

    def __repr__(self):
        return self.name

    def data(self, adt):
        """x, add: flat (tokens C) values of adt; dy (rows, Cw) values of adt, dy32 of fp32; gamma, beta (Cw) values of fp32"""
        g = _gen(self.name)
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        Cw, n = self.Cw, self.tokens * self.C
        gamma, beta = 1.0 + 0.3 * rn(Cw), 0.2 * rn(Cw)
        x = 0.4 + 1.3 * rn(n)
        if self.family == "offset":                                       # |mean| = 30 std: the two-pass variance has to survive it
            x = 30.0 * torch.where(torch.arange(n) // self.C % 2 == 0, 1.0, -1.0).double() + rn(n)
            beta = 3.0 + 0.2 * rn(Cw)                                     # rstd d_mean is 30 (d + 1) u32: keep the outputs away from zero
        elif self.family == "const":
            xr = x.view(-1, self.C)
            xr[0] = 3.0                                                   # variance 0: eps decides
            ulp = 2.0 * torch.finfo(adt).eps                              # spacing of adt in [2, 4)
            xr[1] = 3.0 + ulp * (torch.rand(self.C, generator=g, dtype=torch.float64) < 0.5).double()      # variance of a rounding
        else:
            assert self.family == "plain", self.family
        dy = rn(self.rows, Cw)
        return NS(x=rd(x, adt), add=rd(rn(n), adt), dy=rd(dy, adt), dy32=rd(dy + 1e-3 * rn(self.rows, Cw), None), gamma=rd(gamma, None),
                  beta=rd(beta, None))

    def rows_of(self, x, mut=None):
        return ln_gather(x, self.C, self.merge, self.H, self.W, self.rows, mut)

    def forward(self, d, mut=None):
        return ln_forward(self.rows_of(d.x, mut), d.gamma, d.beta, self.eps, mut)

    def forward_bound(self, d, ref, adt):
        return out_bound(ln_forward_term(self.rows_of(d.x), d.gamma, d.beta, self.eps, self.d), ref, adt)

    def backward(self, d, dy, add, mut=None):
        return ln_backward(d.x, dy, add, d.gamma, self.C, self.merge, self.H, self.W, self.rows, self.eps, mut)

    def backward_bound(self, d, dy, add, ref, adt):
        """flat, x's layout; `written`: the elements the kernel writes"""
        term, _ = ln_backward_term(self.rows_of(d.x), dy, d.gamma, self.eps, self.d)
        idx = ln_source_index(d.x.numel(), self.C, self.merge, self.H, self.W, self.rows).reshape(-1)
        flat = torch.zeros_like(d.x)
        flat[idx] = term.reshape(-1)
        written = torch.zeros(d.x.numel(), dtype=torch.bool)
        written[idx] = True
        assert int(written.sum()) == idx.numel()                          # every source element belongs to exactly one row
        if add is not None:
            flat = flat + U32 * add.abs()
        return out_bound(flat + U32 * ref.abs(), ref, adt), written


def _ln_table():
    cs = []
    for C in (8, 96, 768):
        _, rpb, _ = ln_geom(C)
        for rows in (1, rpb + 1, 2 * rpb + rpb // 2 + 1):                 # one row, one past a workgroup, a partial last workgroup
            cs.append(LnCase(f"ln-c{C}-r{rows}", C, rows, out32=(C == 768 or rows == 1)))
    cs.append(LnCase("ln-c1536-r5", 1536, 5, out32=True))                 # the widest row, 3 chunks on every lane
    for rows in (6, 9, 12):                                               # 4 x 6 grid: 6 rows per image; 9 = rpb + 1 ends inside image 2
        cs.append(LnCase(f"ln-merge-c48-4x6-r{rows}", 48, rows, merge=1, H=4, W=6))
    for rows in (1, 5, 6):
        cs.append(LnCase(f"ln-merge-c384-2x2-r{rows}", 384, rows, merge=1, H=2, W=2))
    cs.append(LnCase("ln-c96-offset", 96, 40, family="offset"))
    cs.append(LnCase("ln-c768-offset", 768, 7, family="offset", out32=True))
    cs.append(LnCase("ln-merge-c48-offset", 48, 12, merge=1, H=4, W=6, family="offset"))
    cs.append(LnCase("ln-c96-const", 96, 40, family="const"))
    cs.append(LnCase("ln-c8-const", 8, 5, family="const", out32=True))
    return cs


LN_CASES = _ln_table()
LN_MUTANTS = {"unbiased": "ln-c8-r257", "eps_outside": "ln-c96-const", "merge_order": "ln-merge-c48-4x6-r12", "swap_hw": "ln-merge-c48-4x6-r12"}
LN_BWD_MUTANTS = {"unbiased": "ln-c8-r257", "merge_order": "ln-merge-c48-4x6-r12", "swap_hw": "ln-merge-c48-4x6-r12", "drop_add": "ln-c96-r17"}


# ================================================================================================================================ GELU
def gelu(u, mut=None):
    if mut == "tanh":
        return 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * u ** 3)))
    return 0.5 * u * torch.erfc(-u / SQRT2)


def _gelu_a1(u):
    z = u / SQRT2
    return ERF_ULP * ULP * torch.erf(z).abs() + 1.5 * U32 * (z * 2.0 / math.sqrt(math.pi) * torch.exp(-z * z)).abs() + U32 * torch.erfc(-z)


def gelu_forward_term(u):
    return 0.5 * u.abs() * _gelu_a1(u) + 2 * U32 * gelu(u).abs() + 2 * UF32


def gelu_backward(u, dy, mut=None):
    ug = u.clone().requires_grad_(True)
    (g,) = torch.autograd.grad((gelu(ug, mut) * dy).sum(), ug)
    return g


def gelu_backward_term(u, dy, ref):
    arg = 0.5 * u * u
    uphi = (u * torch.exp(-arg) / math.sqrt(2.0 * math.pi)).abs()
    dg = 0.5 * torch.erfc(-u / SQRT2) + u * torch.exp(-arg) / math.sqrt(2.0 * math.pi)
    a2 = 0.5 * _gelu_a1(u) + uphi * ((4 * arg + 3) * U32 + EXP_ULP * ULP) + U32 * dg.abs()
    return dy.abs() * a2 + U32 * ref.abs() + 2 * UF32


def gelu_emulate_forward(u, adt):
    x = u.float()
    return rd(0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752)), adt)


def gelu_emulate_backward(u, dy, adt):
    x = u.float()
    df = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)
    return rd(dy.float() * df, adt)


class GeluCase:
    def __init__(self, name, n8, specials_only=False):
        self.name, self.n8, self.exempt = name, n8, specials_only

    def __repr__(self):
        return self.name

    def data(self, adt):
        g = _gen(self.name)
        n = self.n8 * 8
        sub = act_tiny(adt)
        special = torch.tensor([SQRT2, -SQRT2, 0.0, -0.0, sub, -4.0, -5.0, -6.0], dtype=torch.float64)
        if self.exempt:
            u = special
        else:
            grid = torch.linspace(-8.0, 8.0, 97, dtype=torch.float64)     # steps of 1 / 6: the cancellation range -4 .. -6 has 13 points
            u = torch.cat([special, -special[4:5], grid, 1.5 * torch.randn(n - 106, generator=g, dtype=torch.float64)])
        assert u.numel() == n
        dy = torch.randn(n, generator=g, dtype=torch.float64)
        return NS(u=rd(u, adt), dy=rd(dy, adt))


GELU_CASES = [GeluCase("gelu-n8-1", 1, specials_only=True), GeluCase("gelu-n8-255", 255), GeluCase("gelu-n8-257", 257)]
GELU_MUTANTS = {"tanh": "gelu-n8-257"}


# ==================================================================================================================== window attention
def rel_position_index(mut=None):
    """(64, 64) index into the (225, heads) bias table, the Swin way: coordinate differences, shifted to start at 0, row-major"""
    c = torch.stack(torch.meshgrid(torch.arange(WS), torch.arange(WS), indexing="ij")).flatten(1)          # (2, 64)
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0) + (WS - 1)
    if mut == "rel_axes":
        return rel[..., 1] * (2 * WS - 1) + rel[..., 0]
    return rel[..., 0] * (2 * WS - 1) + rel[..., 1]


def region_labels(H, W, shift, mut=None):
    img = torch.zeros(H, W)
    cuts = [slice(0, -WS), slice(-WS, -shift), slice(-shift, None)]
    if mut == "region_bounds":
        cuts = [slice(0, -shift), slice(-shift, -WS), slice(-WS, None)]
    cnt = 0
    for hs in cuts:
        for ws in cuts:
            img[hs, ws] = cnt
            cnt += 1
    return img


def _windows(x, H, W):
    """(B, H, W, ...) -> (B, windows, 64, ...)"""
    B, rest = x.shape[0], x.shape[3:]
    x = x.reshape(B, H // WS, WS, W // WS, WS, -1).permute(0, 1, 3, 2, 4, 5)
    return x.reshape(B, (H // WS) * (W // WS), WT, *rest)


def _unwindows(x, H, W):
    """(B, windows, 64, ...) -> (B, H, W, ...)"""
    B, rest = x.shape[0], x.shape[3:]
    x = x.reshape(B, H // WS, W // WS, WS, WS, -1).permute(0, 1, 3, 2, 4, 5)
    return x.reshape(B, H, W, *rest)


def _win_split(qkv, table, B, H, W, heads, shift, mut=None):
    """-> q, k, v (B, windows, heads, 64, 24), bias (heads, 64, 64), masked (windows, 64, 64) bool or None, the roll to undo"""
    x = qkv.reshape(B, H, W, 3, heads, HD)
    sh = -shift if mut == "roll_plus" else shift
    if shift:
        x = torch.roll(x, shifts=(-sh, -sh), dims=(1, 2))
    xw = _windows(x, H, W).permute(3, 0, 1, 4, 2, 5)                       # (3, B, windows, heads, 64, 24)
    if mut == "bias_layout":
        bias = table.reshape(-1).view(heads, -1)[:, rel_position_index(mut).reshape(-1)].view(heads, WT, WT)
    else:
        bias = table[rel_position_index(mut).reshape(-1)].view(WT, WT, heads).permute(2, 0, 1)
    masked = None
    if shift:
        lab = _windows(region_labels(H, W, shift, mut)[None, :, :, None], H, W)[0, :, :, 0]              # (windows, 64)
        masked = lab[:, :, None] != lab[:, None, :]
    return xw[0], xw[1], xw[2], bias, masked, sh


def _win_merge(o, B, H, W, sh):
    """(B, windows, heads, 64, 24) -> (B, H W, heads 24)"""
    o = _unwindows(o.permute(0, 1, 3, 2, 4), H, W)
    if sh:
        o = torch.roll(o, shifts=(sh, sh), dims=(1, 2))
    return o.reshape(B, H * W, -1)


def win_attn(qkv, table, B, H, W, heads, shift, mut=None):
    """qkv (B, H W, 3 C) float64 -> out (B, H W, C)"""
    if mut == "swap_hw":
        H, W = W, H
    q, k, v, bias, masked, sh = _win_split(qkv, table, B, H, W, heads, shift, mut)
    scale = HD ** -0.5
    s = (q * scale) @ (k * (scale if mut == "scale_both" else 1.0)).transpose(-1, -2) + bias
    if masked is not None:
        s = s + torch.where(masked, 0.0 if mut == "mask_zero" else -100.0, 0.0).double()[None, :, None]
    return _win_merge(torch.softmax(s, -1) @ v, B, H, W, sh)


def win_attn_backward(qkv, dout, table, B, H, W, heads, shift, mut=None):
    x = qkv.clone().requires_grad_(True)
    (g,) = torch.autograd.grad((win_attn(x, table, B, H, W, heads, shift, mut) * dout).sum(), x)
    return g


def _attn_terms(q, k, bias, masked):
    scale = HD ** -0.5
    s = (q * scale) @ k.transpose(-1, -2) + bias
    prod = (q * scale)[..., :, None, :] * k[..., None, :, :]                # (..., 64, 64, 24)
    d_s = U32 * ((bias[..., None] + prod.cumsum(-1)).abs().sum(-1) + 2 * prod.abs().sum(-1))
    if masked is not None:
        m = masked[None, :, None]
        s = s + torch.where(m, -100.0, 0.0).double()
        d_s = d_s + torch.where(m, U32 * s.abs(), torch.zeros((), dtype=torch.float64))
    a = (s - s.max(-1, keepdim=True).values).abs()
    # (the error of the row maximum is common to the row: e_j and their sum carry it alike and p does not see it)
    delta = d_s + U32 * a + EXP_ULP * ULP + 2 * a * U32
    p = torch.softmax(s, -1)
    # the row sum of e, relative to it: a step rounds its partial sum once, and is never off by more than what it adds
    rowsum = torch.minimum(U32 * p.cumsum(-1), p)[..., 1:].sum(-1, keepdim=True)
    return p, delta, (p * delta).sum(-1, keepdim=True), rowsum


def _chain(a, b):
    """first-order error of sum_j a_ij b_jd accumulated by FMAs in the order of j from 0: every step rounds its partial sum once"""
    return U32 * (a[..., :, :, None] * b[..., None, :, :]).cumsum(-2).abs().sum(-2)


def win_attn_forward_bound(qkv, table, ref, B, H, W, heads, shift, adt):
    q, k, v, bias, masked, sh = _win_split(qkv, table, B, H, W, heads, shift)
    p, delta, Delta, rowsum = _attn_terms(q, k, bias, masked)
    term = (p * (delta + Delta)) @ v.abs() + (rowsum + 3 * U32) * (p @ v.abs()) + _chain(p, v) + 2 * UF32
    return out_bound(_win_merge(term, B, H, W, sh), ref, adt)


def win_attn_backward_bound(qkv, dout, table, ref, B, H, W, heads, shift, adt):
    """-> bound of dqkv (B, H W, 3 C): dq | dk | dv each element-wise"""
    q, k, v, bias, masked, sh = _win_split(qkv, table, B, H, W, heads, shift)
    dO = _windows(dout.reshape(B, H, W, heads, HD) if not shift else torch.roll(dout.reshape(B, H, W, heads, HD), (-sh, -sh), (1, 2)), H, W)
    dO = dO.permute(0, 1, 3, 2, 4)
    scale = HD ** -0.5
    p, delta, Delta, rowsum = _attn_terms(q, k, bias, masked)
    # p'_j = p_j (1 + eps_j - sum_k p_k eps_k) (1 + c_j): eps_j the relative error of e_j (|eps_j| <= delta_j), c_j the row sum, 1 / sum
    # and the product (|c_j| <= kap).  The eps part keeps sum_j p_j = 1, so in delta = sum_j p_j dP_j it leaves sum_j eps_j dS_j, not
    # sum_j |p_j eps_j dP_j|: a near one-hot row (dS small beside p dP) keeps its resolution
    kap = rowsum + 3 * U32
    e_p = p * (delta + Delta - 2 * p * delta + kap)
    vt = v.transpose(-1, -2)
    dP, e_dP = dO @ vt, _chain(dO, vt)
    dl = (p * dP).sum(-1, keepdim=True)
    w = dP - dl
    dS = p * w
    e_dl = (delta * dS.abs() + kap * p * dP.abs() + p * e_dP).sum(-1, keepdim=True) + U32 * (p * dP).cumsum(-1).abs().sum(-1, keepdim=True)
    e_dS = dS.abs() * (delta + Delta + kap) + p * (e_dP + e_dl + U32 * w.abs()) + U32 * dS.abs()
    dSt, pt = dS.transpose(-1, -2), p.transpose(-1, -2)
    b_dq = scale * (e_dS @ k.abs() + _chain(dS, k)) + 2 * U32 * scale * (dS.abs() @ k.abs())
    b_dk = scale * (e_dS.transpose(-1, -2) @ q.abs() + _chain(dSt, q)) + 2 * U32 * scale * (dSt.abs() @ q.abs())
    b_dv = e_p.transpose(-1, -2) @ dO.abs() + _chain(pt, dO)
    term = torch.stack([_win_merge(t, B, H, W, sh) for t in (b_dq, b_dk, b_dv)], 2).reshape(B, H * W, -1) + 4 * UF32
    return out_bound(term, ref, adt)


def win_attn_emulate(qkv, dout, table, B, H, W, heads, shift, adt):
    """fp32: scores by the scaled q, the -100 added to the score, exp of the difference to the row maximum, one division per row ->
    (out, dqkv) as float64 values of adt"""
    q, k, v, bias, masked, sh = _win_split(qkv.float(), table.float(), B, H, W, heads, shift)
    scale = torch.tensor(0.20412414523193154, dtype=torch.float32)
    qs = q * scale
    s = qs @ k.transpose(-1, -2) + bias
    if masked is not None:
        s = torch.where(masked[None, :, None], s + torch.tensor(-100.0), s)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    inv = 1.0 / e.sum(-1, keepdim=True, dtype=torch.float32)
    out = _win_merge((e @ v) * inv, B, H, W, sh)
    d5 = dout.float().reshape(B, H, W, heads, HD)
    dO = _windows(torch.roll(d5, (-sh, -sh), (1, 2)) if shift else d5, H, W).permute(0, 1, 3, 2, 4)
    p = e * inv
    dP = dO @ v.transpose(-1, -2)
    dS = p * (dP - (p * dP).sum(-1, keepdim=True, dtype=torch.float32))
    dq, dk, dv = (dS @ k) * scale, dS.transpose(-1, -2) @ qs, p.transpose(-1, -2) @ dO
    dqkv = torch.stack([_win_merge(t, B, H, W, sh) for t in (dq, dk, dv)], 2).reshape(B, H * W, -1)
    return rd(out, adt), rd(dqkv, adt)


class AttnCase:
    def __init__(self, name, B, H, W, heads, shift, family="plain"):
        self.name, self.B, self.H, self.W, self.heads, self.shift, self.family = name, B, H, W, heads, shift, family
        self.C = heads * HD

    def __repr__(self):
        return self.name

    @property
    def geom(self):
        return self.B, self.H, self.W, self.heads, self.shift

    def data(self, adt):
        """qkv (B, H W, 3 C), dout (B, H W, C) values of adt; table (225, heads) values of fp32"""
        g = _gen(self.name)
        B, H, W, heads, C = self.B, self.H, self.W, self.heads, self.C
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        qkv = rn(B, H * W, 3, heads, HD)
        qkv[:, :, 2] += 0.5                                                # v with a common part: fewer outputs that cancel to nothing
        table = 0.5 * rn((2 * WS - 1) ** 2, heads)
        if self.family == "peaked":
            qkv[:, :, 0] *= 6.0                                            # softmax near one-hot
        elif self.family == "competitive":
            # a query and a key of ANOTHER shift region in one window: q . k / sqrt 24 = +60 (and +97 for a second pair), so that the
            # masked logit sits at -40 (-3) beside unmasked ones around 0: the -100 has to win by what the model says, not by more
            tok = _windows(torch.roll(torch.arange(H * W).view(1, H, W, 1), (-self.shift, -self.shift), (1, 2)), H, W)[0, :, :, 0]
            lab = _windows(region_labels(H, W, self.shift)[None, :, :, None], H, W)[0, :, :, 0]
            win = tok.shape[0] - 1                                         # the last window holds four regions
            for pair, target in ((0, 60.0), (1, 97.0)):
                i = 9 * pair
                j = int((lab[win] != lab[win, i]).nonzero()[pair * 3])
                val = math.sqrt(target * math.sqrt(HD) / HD)
                qkv[:, tok[win, i], 0, 0] = val
                qkv[:, tok[win, j], 1, 0] = val
        else:
            assert self.family == "plain", self.family
        return NS(qkv=rd(qkv.reshape(B, H * W, 3 * C), adt), dout=rd(rn(B, H * W, C), adt), table=rd(table, None))


ATTN_CASES = [AttnCase("attn-one-window", 1, 8, 8, 1, 0), AttnCase("attn-16x16-shift", 2, 16, 16, 2, 4),
              AttnCase("attn-16x24-shift", 1, 16, 24, 2, 4), AttnCase("attn-24x16-shift", 1, 24, 16, 3, 4),
              AttnCase("attn-16x16-noshift", 2, 16, 16, 2, 0), AttnCase("attn-peaked", 1, 16, 16, 2, 4, family="peaked"),
              AttnCase("attn-competitive", 1, 16, 16, 2, 4, family="competitive")]
ATTN_MUTANTS = {"roll_plus": "attn-16x24-shift", "region_bounds": "attn-16x16-shift", "mask_zero": "attn-16x16-shift",
                "rel_axes": "attn-one-window", "bias_layout": "attn-16x16-noshift", "scale_both": "attn-one-window",
                "swap_hw": "attn-16x24-shift"}


# =============================================================================================================================== embed
def bicubic_taps(frames, Tout, mut=None, index_dtype=torch.float32):
    """-> (idx (Tout, 4) long, w (Tout, 4) float64): torch's bicubic taps along one axis with align_corners = True.  The source index is
    computed in `index_dtype` (float32: what a float32 network does; the float64 cross-check against torch passes float64)."""
    A = -0.5 if mut == "cubic_a" else -0.75
    t = torch.arange(Tout, dtype=index_dtype)
    if frames == Tout:
        src = t
    elif mut == "half_pixel":                                              # align_corners = False
        src = torch.tensor(frames, dtype=index_dtype) / torch.tensor(Tout, dtype=index_dtype) * (t + 0.5) - 0.5
    else:
        src = torch.tensor(frames - 1, dtype=index_dtype) / torch.tensor(Tout - 1, dtype=index_dtype) * t
    i0 = src.floor()
    fr = (src - i0).double()
    c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
    c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    w = torch.stack([c2(fr + 1), c1(fr), c1(1 - fr), c2(2 - fr)], 1)
    idx = i0.long()[:, None] + torch.arange(-1, 3)
    if mut == "no_clamp":                                                  # taps outside the signal read zeros
        w = torch.where((idx >= 0) & (idx < frames), w, torch.zeros((), dtype=torch.float64))
    return idx.clamp(0, frames - 1), w


def fold_image(X, spec, bins, mut=None):
    """(B, Tout, bins) -> (B, spec, spec): img[c bins + f][tt] = X[c T + tt][f]"""
    B, ratio = X.shape[0], spec // bins
    x4 = X.reshape(B, ratio, spec, bins)
    if mut == "fold_cf":
        return x4.permute(0, 3, 1, 2).reshape(B, spec, spec)               # img[f ratio + c][tt]
    return x4.permute(0, 1, 3, 2).reshape(B, spec, spec)


def unfold_image(img, spec, bins):
    B, ratio = img.shape[0], spec // bins
    return img.reshape(B, ratio, bins, spec).permute(0, 1, 3, 2).reshape(B, ratio * spec, bins)


def stretch(x, idx, w):
    """(B, frames, bins) -> (B, Tout, bins)"""
    return (x[:, idx] * w[None, :, :, None]).sum(2)


def embed_forward(mel, P, cfg, z0=None, mut=None, index_dtype=torch.float32):
    """mel (B, frames, bins) float64 -> tokens (B, (spec / 4)^2, E).  z0: a zero tensor at the stretched image (its gradient is `dimg`)"""
    B, frames, bins = mel.shape
    Tout = cfg.spec * (cfg.spec // bins)
    a = P.bn_w / torch.sqrt(P.bn_v + (0.0 if mut == "bn_eps" else cfg.bn_eps))
    x = (mel - P.bn_m) * a + P.bn_b
    X = stretch(x, *bicubic_taps(frames, Tout, mut, index_dtype))
    if z0 is not None:
        X = X + a * z0
    img = fold_image(X, cfg.spec, bins, mut)
    conv = F.conv2d(img[:, None], P.Wp, P.bp, stride=4).flatten(2).transpose(1, 2)
    return F.layer_norm(conv, (cfg.E,), P.ln_g, P.ln_b, cfg.ln_eps)


def embed_backward(mel, dtok, scale, P, cfg, mut=None):
    """-> (dimg (B, Tout, bins), dmel (B, frames, bins)) by autograd"""
    B, frames, bins = mel.shape
    m = mel.clone().requires_grad_(True)
    z0 = torch.zeros(B, cfg.spec * (cfg.spec // bins), bins, dtype=torch.float64, requires_grad=True)
    dimg, dmel = torch.autograd.grad((embed_forward(m, P, cfg, z0, mut) * dtok).sum(), (z0, m))
    if scale is not None:
        dmel = dmel * scale[:, None, None]
    return dimg, dmel


def _embed_parts(mel, P, cfg):
    """the chain's magnitudes: conv (B, tokens, E) and its carried error e_conv"""
    B, frames, bins = mel.shape
    Tout = cfg.spec * (cfg.spec // bins)
    idx, w = bicubic_taps(frames, Tout)
    a = P.bn_w / torch.sqrt(P.bn_v + cfg.bn_eps)
    pix = stretch((mel - P.bn_m) * a + P.bn_b, idx, w)
    d_pix = 7 * U32 * a.abs() * stretch(mel.abs(), idx, w.abs()) + U32 * (P.bn_b.abs() + 3 * (P.bn_m * a).abs()) + U32 * pix.abs()
    img, d_img = fold_image(pix, cfg.spec, bins), fold_image(d_pix, cfg.spec, bins)
    tok = lambda t: t.flatten(2).transpose(1, 2)
    conv = tok(F.conv2d(img[:, None], P.Wp, P.bp, stride=4))
    e_conv = tok(F.conv2d(d_img[:, None], P.Wp.abs(), None, stride=4)) + 17 * U32 * tok(F.conv2d(img.abs()[:, None], P.Wp.abs(), P.bp.abs(), stride=4))
    return NS(conv=conv, e_conv=e_conv, a=a, idx=idx, w=w, Tout=Tout)


def embed_forward_bound(mel, P, cfg, ref, adt):
    s = _embed_parts(mel, P, cfg)
    E = cfg.E
    term = ln_forward_term(s.conv.reshape(-1, E), P.ln_g, P.ln_b, cfg.ln_eps, E, s.e_conv.reshape(-1, E)).reshape(ref.shape)
    return out_bound(term, ref, adt)


def embed_backward_bound(mel, dtok, scale, P, cfg, dimg_ref, dmel_ref):
    """-> (bound of dimg, bound of dmel), both fp32 outputs"""
    B, frames, bins = mel.shape
    s = _embed_parts(mel, P, cfg)
    E, g = cfg.E, cfg.spec // 4
    e_dpre, dpre = ln_backward_term(s.conv.reshape(-1, E), dtok.reshape(-1, E), P.ln_g, cfg.ln_eps, E, s.e_conv.reshape(-1, E))
    e_dpre = e_dpre + U32 * dpre.abs()
    grid = lambda t: t.reshape(B, g, g, E).permute(0, 3, 1, 2)
    Wa = P.Wp.abs()
    e_dp = F.conv_transpose2d(grid(e_dpre), Wa, stride=4) + E * U32 * F.conv_transpose2d(grid(dpre.abs()), Wa, stride=4)
    b_dimg = s.a.abs() * unfold_image(e_dp[:, 0], cfg.spec, bins) + 2 * U32 * dimg_ref.abs() + 2 * UF32
    # transposed stretch: frame k sums the n_k taps that read it
    flat = s.idx.reshape(-1)
    wa = s.w.abs()[None, :, :, None]
    pull = lambda t: torch.zeros(B, frames, bins, dtype=torch.float64).index_add_(1, flat, (t[:, :, None, :] * wa).reshape(B, -1, bins))
    n_k = torch.zeros(frames, dtype=torch.float64).index_add_(0, flat, (s.w != 0).double().reshape(-1))
    b_dmel = pull(b_dimg) + (n_k[None, :, None] + 3) * U32 * pull(dimg_ref.abs())
    if scale is not None:
        b_dmel = b_dmel * scale.abs()[:, None, None]
    return b_dimg, b_dmel + U32 * dmel_ref.abs() + 2 * UF32


def embed_emulate(mel, dtok, scale, P, cfg, adt):
    """fp32: BatchNorm folded to a x + c and applied after the stretch, the convolution, a two-pass LayerNorm; the backward sums; the
    transposed stretch; the scale last -> (tokens values of adt, dimg, dmel values of fp32)"""
    B, frames, bins = mel.shape
    E, g = cfg.E, cfg.spec // 4
    f = lambda t: t.float()
    idx, w = bicubic_taps(frames, cfg.spec * (cfg.spec // bins))
    a = f(P.bn_w / torch.sqrt(P.bn_v + cfg.bn_eps))
    c = f(P.bn_b) - f(P.bn_m) * a
    pix = a * stretch(f(mel), idx, f(w)) + c
    conv = F.conv2d(fold_image(pix, cfg.spec, bins)[:, None], f(P.Wp), f(P.bp), stride=4).flatten(2).transpose(1, 2)
    mean = conv.sum(-1, keepdim=True, dtype=torch.float32) / E
    dd = conv - mean
    rstd = torch.rsqrt((dd * dd).sum(-1, keepdim=True, dtype=torch.float32) / E + torch.tensor(cfg.ln_eps, dtype=torch.float32))
    xh = dd * rstd
    tokens = rd(xh * f(P.ln_g) + f(P.ln_b), adt)
    gg = f(dtok) * f(P.ln_g)
    mg, mgx = gg.sum(-1, keepdim=True, dtype=torch.float32) / E, (gg * xh).sum(-1, keepdim=True, dtype=torch.float32) / E
    dpre = rstd * (gg - mg - xh * mgx)
    dp = F.conv_transpose2d(dpre.reshape(B, g, g, E).permute(0, 3, 1, 2), f(P.Wp), stride=4)
    dimg = a * unfold_image(dp[:, 0], cfg.spec, bins)
    dmel = torch.zeros(B, frames, bins).index_add_(1, idx.reshape(-1), (dimg[:, :, None, :] * f(w)[None, :, :, None]).reshape(B, -1, bins))
    if scale is not None:
        dmel = dmel * f(scale)[:, None, None]
    return tokens, dimg.double(), dmel.double()


EMBED_CFG = dict(spec=64, bins=32, ln_eps=1e-5, bn_eps=1e-5)                # Tout = 128, a 16 x 16 token grid, two time chunks
EMBED_SMALL_VAR_BINS = (5,)                                                # running_var a hundred times the BatchNorm eps


def embed_config(E):
    return NS(E=E, **EMBED_CFG)


def embed_params(E):
    """parameters of the input stage as float64 values of fp32; BatchNorm statistics far from identity"""
    g = _gen(f"embed-params-{E}")
    bins = EMBED_CFG["bins"]
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    bn_v = 150.0 * (1.0 + 0.3 * torch.rand(bins, generator=g, dtype=torch.float64))
    bn_m = -20.0 + 3.0 * rn(bins)
    for f in EMBED_SMALL_VAR_BINS:
        # eps = 1e-5 is 1 % of this variance (the bin stays close to its mean).  A mean of -2: the folded BatchNorm computes a x + (b - m a),
        # which cancels to |m a| u32; with m = -20 here the tokens of this bin's row could not be sharp
        bn_v[f], bn_m[f] = 1e-3, -2.0
    P = NS(bn_w=1.0 + 0.2 * rn(bins), bn_b=0.1 * rn(bins), bn_m=bn_m, bn_v=bn_v, Wp=0.25 * rn(E, 1, 4, 4),
           bp=0.1 * rn(E), ln_g=1.0 + 0.2 * rn(E), ln_b=0.1 * rn(E))
    return NS(**{k: rd(v, None) for k, v in vars(P).items()})


class EmbedCase:
    def __init__(self, E, frames, with_scale, B=2):
        self.name = f"embed-e{E}-f{frames}-{'scale' if with_scale else 'noscale'}"
        self.E, self.frames, self.with_scale, self.B = E, frames, with_scale, B

    def __repr__(self):
        return self.name

    def data(self, adt):
        """mel (B, frames, bins), scale (B) or None: values of fp32; dtok (B, 256, E) values of adt"""
        g = _gen(self.name)
        bins, P = EMBED_CFG["bins"], embed_params(self.E)
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        t = torch.arange(self.frames, dtype=torch.float64)[None, :, None]
        f = torch.arange(bins, dtype=torch.float64)[None, None, :]
        mel = -25.0 + 12.0 * torch.sin(0.35 * t + 0.3 * f) + 0.25 * f + 6.0 * rn(self.B, self.frames, bins)      # a per-bin pattern
        for k in EMBED_SMALL_VAR_BINS:
            mel[:, :, k] = P.bn_m[k] + 0.03 * (1.0 + rn(self.B, self.frames))
        scale = torch.tensor([0.5, 2.0], dtype=torch.float64)[:self.B] if self.with_scale else None
        return NS(mel=rd(mel, None), dtok=rd(rn(self.B, (EMBED_CFG["spec"] // 4) ** 2, self.E), adt), scale=scale, P=P)


EMBED_FRAMES = [2, 3, 100, 127, 128]
EMBED_CASES = [EmbedCase(E, fr, (i + (E == 128)) % 2 == 0) for E in (8, EMB_MAX) for i, fr in enumerate(EMBED_FRAMES)]
EMBED_MUTANTS = {"cubic_a": "embed-e8-f100-scale", "half_pixel": "embed-e8-f100-scale", "no_clamp": "embed-e8-f3-noscale",
                 "fold_cf": "embed-e8-f128-scale", "bn_eps": "embed-e8-f128-scale"}


# ================================================================================================================================ Gram
def gram(Fm, mut=None):
    T, C = Fm.shape[1:]
    return Fm.transpose(1, 2) @ Fm / (C if mut == "gram_over_c" else T)


def gram_backward(Fm, dG, mut=None):
    if mut == "gram_no_transpose":
        return Fm @ dG / Fm.shape[1]
    x = Fm.clone().requires_grad_(True)
    (g,) = torch.autograd.grad((gram(x, mut) * dG).sum(), x)
    return g


def gram_bounds(Fm, dG):
    T, C = Fm.shape[1:]
    a = Fm.abs()
    return (T + 2) * U32 * (a.transpose(1, 2) @ a) / T + 2 * UF32, (C + 3) * U32 * (a @ (dG.abs() + dG.abs().transpose(1, 2))) / T + 2 * UF32


def gram_emulate(Fm, dG):
    """fp32; the 1 / T is applied after the sum"""
    f, g = Fm.float(), dG.float()
    inv = torch.tensor(1.0, dtype=torch.float32) / Fm.shape[1]
    return ((f.transpose(1, 2) @ f) * inv).double(), ((f @ (g + g.transpose(1, 2))) * inv).double()


class GramCase:
    def __init__(self, B, T, C):
        self.name, self.B, self.T, self.C = f"gram-b{B}-t{T}-c{C}", B, T, C

    def __repr__(self):
        return self.name

    def data(self):
        g = _gen(self.name)
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        return NS(F=rd(0.3 + rn(self.B, self.T, self.C), None), dG=rd(rn(self.B, self.C, self.C), None))       # dG is not symmetric


GRAM_CASES = [GramCase(2, 1, 4), GramCase(1, 33, 70), GramCase(2, 64, 128), GramCase(1, 96, 65)]
GRAM_MUTANTS = {"gram_over_c": "gram-b1-t33-c70", "gram_no_transpose": "gram-b1-t33-c70"}
GRAM_MAX_T = 96
