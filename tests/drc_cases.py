"""Shared by tests/test_drc_bound_host.py (CPU) and tests/test_gpu_drc.py (GPU): a float64 model of the dynamic-range compressor and of the
transpose of its Jacobian (csrc/drc.hip), an element-wise bound, an fp32 emulation in the kernels' documented order,
mutants and the case table.  Written the way tests/tf_gain_cases.py and tests/spectral_cases.py are; no GPU dependency.

MODEL (float64, from the definition; `model`, `model_bwd`).  The definition, as DESIGN.md section 8.9 has it:

    Everything is per clip. `x` is zero outside `[0, L)`. The sidechain runs at block rate `R = 64` samples (4 ms at 16 kHz).

    - **Why block rate.** The attack/release follower is not an associative scan. Its step is the maximum (or minimum) of two affine maps of the state. So the follower is a true serial chain. At block rate it has `H = ceil(L / 64)` steps, 2500 for 10 s, and not 160 000.

    Parameters, shared by all clips:
    - threshold `T` (dB)
    - `ratio >= 1`, where `inf` gives a limiter. `k = 1 - 1/ratio`.
    - knee width `W >= 0` (dB)
    - `attack_ms`, `release_ms > 0`
    - `makeup_db`
    - `eps = 1e-10`

    The follower coefficients are `aA = 1 - exp(-R / (fs * tA))` and `aR` likewise. Compute them on the host in float64 and round once to fp32. Kernel and model then use the same fp32 constants.

    1. **Block power.** `p[j] = (1/64) sum_{r<64} x[64 j + r]^2`, for `j = 0 .. H-1`.
    2. **Level.** `l[j] = 10 log10(p[j] + eps)` and `d = l - T`.
    3. **Static curve, region `rg[j]`.**
       - Region 0, if `2d < -W`: `c = 0`.
       - Region 1, else if `2d <= W`: `c = k (d + W/2)^2 / (2W)`.
       - Region 2, otherwise: `c = k d`.
       - With `W = 0`, region 1 is empty, so `c = k max(d, 0)`.
    4. **Follower on the gain reduction, in dB.** `s[-1] = 0`. `att[j] = (c[j] > s[j-1])`. `s[j] = s[j-1] + (att[j] ? aA : aR) (c[j] - s[j-1])`.
    5. **Block gain.** `G[j] = 10^((makeup_db - s[j]) / 20)` and `G[-1] = 10^(makeup_db / 20)`.
    6. **Output.** `g[64 j + r] = G[j-1] + ((r+1)/64) (G[j] - G[j-1])`. The weights are exact in fp32. `y[n] = g[n] x[n]` for `n < L`.

    **Transpose of the Jacobian at `x`.**
    - Let `w_r = (r+1)/64` and `q[n] = dy[n] x[n]`.
    - `dG[j] = sum_r q[64j+r] w_r + sum_r q[64(j+1)+r] (1 - w_r)`. The second sum is absent for `j = H-1`.
    - `ds[j] = -(ln 10 / 20) G[j] dG[j]`.
    - Backwards from `j = H-1` with `carry = 0`:
      - `tot = ds[j] + carry`
      - `dc[j] = a_j tot`
      - `carry = (1 - a_j) tot`
      - `a_j` is `aA` or `aR` according to `att[j]`.
    - `c'` is `0`, `k (d + W/2) / W` or `k` according to `rg[j]`.
    - `dp[j] = dc[j] c'[j] (10 / ln 10) / (p[j] + eps)`.
    - `dx[n] = g[n] dy[n] + dp[j] (2/64) x[n]`, with zeros on `[L, full)`.

  The model takes T, k, W, aA, aR and makeup_db as float64 values of fp32 numbers.  With W = 0 a block with d = 0 exactly lands in region 1 with
  c = 0 and c' = 0, on both sides.  The transpose is checked against a float64 central difference in the host test.
  `model_bwd` takes the TAPE (one byte per block: bits 0-1 rg, bit 2 att) as an argument: the kernel's backward never re-decides a gate, so
  it is judged against the model run with the kernel's own tape.

BOUND, from the number formats alone (u = 2^-24, gamma(n) = n u / (1 - n u); `bound`, `bound_bwd`), a componentwise absolute-value
propagation of the model; it holds with and without FMA contraction (an FMA has fewer roundings).
    inputs    x, dy are fp32: exact.  The constants kq = k / (2 W), 1 - aA, 1 - aR, 10 / ln 10, ln 10 / 20, 1 / 20 are rounded once (u each)
    power     squares (u each) summed 7 additions deep (3 in the lane, 4 butterfly levels), all terms >= 0: b_p = gamma(8) p; 1 / 64 is exact
    level     arg = p + eps (eps rounded, the sum rounded); log10f ASSUMED within ULP_LOG = 2 ulp as in spectral_cases.py (same source, same
              caveat: the routine is the ROCm device library's, not measured here); times 10 and minus T, one rounding each -> b_d
    curve     c is continuous across both gates and k-Lipschitz in d: b_c = k b_d + kq (2 b_d)^2 (the branches differ by k e^2 / (2 W) at
              distance e from a gate) + gamma(6) (|c| + k b_d) (constant, t = d + W/2, two products).  A block in region 0 that is not
              ambiguous has c = 0 exactly on both sides: b_c = 0
    follower  s' = (1 - a) s + a c with a chosen by the sign of c - s is continuous:
              b_s[j] <= max(1-aA, 1-aR) b_s[j-1] + max(aA, aR) b_c[j] + u (2 max(aA, aR) (|c - s| + b_c + b_s[j-1]) + |s[j]| + the two terms before)
              where the block is ambiguous (see GATES).  Where it is not, both sides take the model's branch a_j, and (1 - a_j) and a_j stand
              in place of the two maxima: never more, and what keeps b_s from outliving s when the release is the faster of the two.  Every
              step with a non-zero operand also adds TINY = 2^-126, the most a rounding can lose below the normal range, flushed or not
    gain      t = (makeup - s) / 20: b_t = b_s / 20 + gamma(3) (|t| + b_s / 20); exp10f ASSUMED within ULP_EXP = 2 ulp (ROCm documents 1):
              b_G = G (expm1(ln 10 b_t) + 2 ULP_EXP u exp(ln 10 b_t))
    output    g = Gp + w (Gc - Gp) is a convex combination: b_g = (1 - w) b_Gp + w b_Gc + gamma(3) (|Gp| + |Gc| + b_Gp + b_Gc); y = g x: one rounding
    transpose q (u), the weighted terms (2 u), sums 7 deep, one more addition: b_dG = gamma(11) (sum |q| w + sum |q'| (1 - w));
              ds: three roundings on top of b_G and b_dG; the backward chain as the forward one, with the tape's a_j (no gate, no max);
              c': exact in regions 0 and 2, 2 kq (d + W/2) in region 1 from b_d; dp: four roundings and the relative error of p + eps;
              dx = g dy + dp' x: gamma(3) on both terms
GATES: the forward is continuous across both gates, so EVERY element of y, s and G must lie inside the bound -- no ambiguous share.  A tape
bit may differ from the model's only where the model is ambiguous: |c[j] - s[j-1]| <= b_c[j] + b_s[j-1] for att, 2 d within 2 b_d of +-W for rg.
Blocks with c = 0 and s = 0 exact on both sides (b_c + b_s = 0) are not ambiguous: 0 > 0 is false on both.  Given the kernel's tape, every
element of dx must lie inside the bound.  CAP: ambiguous blocks are at most AMBIG_CAP = 1 % of a case's blocks, none for cases with H < 100;
asserted from the float64 model alone.

EMULATION (`emulate`, `emulate_bwd`): numpy float32 in the kernels' order -- a lane adds its four terms left to right, the 16 lanes of a block
add pairwise over lane distances 1, 2, 4, 8; no FMA.  It validates the bound on the CPU; it is not a second oracle.

MUTANTS: `MUTANTS` maps a name to (stage, case names); each must leave the bound in at least one element of one listed case.  No mutant was
found that no input separates.

CASES: see `CASES`; every case carries `why`.  Inputs are seeded gated noise: an envelope that switches between about -34 dBFS and about
-6 dBFS every ~1000 samples, times randn."""
import math
import zlib
from types import SimpleNamespace

import numpy as np

from tests import spectral_cases as S

U, gamma, ratio, ULP_LOG = S.U, S.gamma, S.ratio, S.ULP_LOG
ULP_EXP = 2.0
AMBIG_CAP = 0.01
f32, f64 = np.float32, np.float64
R = 64
EPS = 1e-10
C10 = 10.0 / math.log(10.0)
LN10_20 = math.log(10.0) / 20.0
FS = 16000
TINY = 2.0 ** -126


def blocks(L):
    return -(-L // R)


# ------------------------------------------------------------------------------------------------------------------ parameters
def params(threshold_db=-24.0, ratio=4.0, knee_db=6.0, attack_ms=5.0, release_ms=100.0, makeup_db=0.0):
    """the six fp32 parameters the kernels take, as float64 values of fp32 numbers, and what the model derives from them in float64"""
    from diffmusic_amd.inverse_problem.dsp import drc_coeffs
    aA, aR = drc_coeffs(FS, attack_ms, release_ms)
    T, W, mk, k = float(f32(threshold_db)), float(f32(knee_db)), float(f32(makeup_db)), float(f32(1.0 - 1.0 / ratio))
    aA, aR = float(aA), float(aR)
    return SimpleNamespace(T=T, k=k, W=W, aA=aA, aR=aR, makeup=mk, kq=k / (2.0 * W) if W > 0 else 0.0, args=(T, k, W, aA, aR, mk))


PARAMS = {"base": params(), "hard": params(knee_db=0.0), "limiter": params(ratio=math.inf), "fastrel": params(attack_ms=50.0, release_ms=2.0),
          "makeup": params(makeup_db=7.5, ratio=8.0), "quiet": params(makeup_db=-3.0)}


# ------------------------------------------------------------------------------------------------------------------ cases and inputs
def _case(name, why, L, par="base", B=3, full=None, stride=None, off=0, signal="gated"):
    full = full or L
    return SimpleNamespace(name=name, why=why, L=L, H=blocks(L), par=par, P=PARAMS[par], B=B, full=full, stride=stride or full, off=off, signal=signal)


CASES = [
    _case("L1", "a single sample: one block of one", 1),
    _case("L63", "one block, one sample short", 63),
    _case("L64_hard", "exactly one block; hard knee", 64, "hard"),
    _case("L65", "one block and one sample: G[-1] and two blocks", 65, full=70),
    _case("L1000", "a partial last block of 40 samples, less than one workgroup", 1000, full=1003),
    _case("L1000_hard", "the same with W = 0", 1000, "hard"),
    _case("L6400", "H = 100, seven workgroups; the step tests' length", 6400),
    _case("L6400_hard", "W = 0", 6400, "hard"),
    _case("L6400_limiter", "ratio = inf: k = 1", 6400, "limiter"),
    _case("L6400_fastrel", "release faster than attack: aA < aR", 6400, "fastrel"),
    _case("L6400_makeup", "makeup_db = 7.5, ratio 8, Lfull > L", 6400, "makeup", full=6432),
    _case("L6400_quiet", "every block below the knee: y = makeup x, the tape all zero", 6400, "quiet", signal="quiet"),
    _case("L6400_silence", "all zeros", 6400, signal="silence"),
    _case("L20037_stride", "odd length, an unaligned row offset (scalar loads), row stride above L, Lfull > L", 20037, full=20100, stride=20101, off=1),
    _case("L20037_hard_aligned", "the same length on aligned rows (float4 loads) with a stride above L; W = 0", 20037, "hard", stride=20040),
    _case("L70000", "H = 1094: crosses every chunk of the follower", 70000),
    _case("L70000_fastrel", "H = 1094 with aA < aR", 70000, "fastrel", full=70001),
]
CASE = {c.name: c for c in CASES}


def _rng(name, tag):
    return np.random.default_rng(zlib.crc32(f"drc/{name}/{tag}".encode()))


def gated_noise(rng, n, lo_db=-34.0, hi_db=-6.0):
    """an envelope that switches between lo_db and hi_db (dBFS, rms) every 700 .. 1300 samples, times randn"""
    env = np.empty(n)
    i, loud = 0, bool(rng.integers(2))
    while i < n:
        seg = int(rng.integers(700, 1301))
        env[i:i + seg] = 10.0 ** ((hi_db if loud else lo_db) / 20.0)
        i, loud = i + seg, not loud
    return env * rng.standard_normal(n)


_INPUTS = {}


def inputs(c):
    """everything a case feeds the kernels, fp32 numpy, identical on the host and the GPU side; cached and never modified"""
    if c.name not in _INPUTS:
        rng = _rng(c.name, "x")
        if c.signal == "gated":
            store = np.stack([gated_noise(rng, c.stride) for _ in range(c.B)])
        elif c.signal == "quiet":
            store = 10.0 ** (-40.0 / 20.0) * rng.standard_normal((c.B, c.stride))
        else:
            store = np.zeros((c.B, c.stride))
        store = store.astype(f32)
        dy = _rng(c.name, "dy").standard_normal((c.B, c.L)).astype(f32)
        _INPUTS[c.name] = SimpleNamespace(store=store, x=store[:, :c.L], dy=dy)
    return _INPUTS[c.name]


# ------------------------------------------------------------------------------------------------------------------ float64 model
def _blocked(v, L, dtype=f64):
    """(B, >= L) -> (B, H, 64), zero past L"""
    B, H = v.shape[0], blocks(L)
    out = np.zeros((B, H * R), dtype)
    out[:, :L] = v[:, :L]
    return out.reshape(B, H, R)


def curve(d, P):
    """-> (rg, c) of the static curve at d = level - T"""
    rg = np.where(2.0 * d < -P.W, 0, np.where(2.0 * d <= P.W, 1, 2))
    t = d + 0.5 * P.W
    c = np.where(rg == 0, 0.0, np.where(rg == 1, P.kq * t * t, P.k * d))
    return rg, c


def slope(d, rg, P, mut=None):
    knee = 2.0 * P.kq * (d + 0.5 * P.W)
    return np.where(rg == 0, 0.0, np.where((rg == 1) | (mut == "knee_slope_above_knee"), knee, P.k))


def interp(G, makeup, L, mut=None, dtype=f64):
    """block gains (B, H) -> g (B, L)"""
    B, H = G.shape
    G0 = np.full((B, 1), 10.0 ** (makeup / 20.0), dtype) if dtype is f64 else np.power(f32(10), np.full((B, 1), f32(makeup) * f32(0.05), f32))
    Gp = G if mut == "no_interpolation" else np.concatenate([G0, G[:, :-1]], axis=1)
    w = ((np.arange(R) + (0 if mut == "weight_r_over_64" else 1)) / R).astype(dtype)
    return (Gp[..., None] + w * (G - Gp)[..., None]).reshape(B, H * R)[:, :L]


def model(x, L, P, mut=None):
    """float64 forward: x (B, >= L) -> namespace with every intermediate; r.y (B, L), r.tape (B, H) uint8"""
    x = np.asarray(x, f64)[:, :L]
    B, H = x.shape[0], blocks(L)
    r = SimpleNamespace(H=H)
    xb = _blocked(x, L)
    r.p = (xb * xb).sum(-1) / R
    if mut == "partial_block_own_mean":
        r.p[:, -1] = (xb[:, -1] ** 2).sum(-1) / (L - (H - 1) * R)
    r.arg = r.p + EPS
    r.l = 10.0 * np.log10(r.arg)
    r.d = r.l - P.T
    r.rg, r.c = curve(r.d, P)
    r.s, r.att, r.sprev = np.zeros((B, H)), np.zeros((B, H), bool), np.zeros((B, H))
    s = np.zeros(B)
    for j in range(H):
        r.sprev[:, j] = s
        r.att[:, j] = r.c[:, j] > s
        s = s + np.where(r.att[:, j], P.aA, P.aR) * (r.c[:, j] - s)
        r.s[:, j] = s
    r.G = 10.0 ** ((P.makeup - r.s) / 20.0)
    r.g = interp(r.G, P.makeup, L, mut)
    r.y = r.g * x
    r.tape = (r.rg | (r.att.astype(np.int64) << 2)).astype(np.uint8)
    return r


def model_bwd(x, dy, L, P, r, tape, mut=None):
    """float64 transpose of the Jacobian at x with the gates of `tape` -> namespace; rb.dx (B, L)"""
    x, dy = np.asarray(x, f64)[:, :L], np.asarray(dy, f64)[:, :L]
    B, H = x.shape[0], blocks(L)
    p, G = r.p, r.G
    if mut == "state_of_clip_0":
        p, G = np.broadcast_to(p[:1], p.shape), np.broadcast_to(G[:1], G.shape)
    rb = SimpleNamespace()
    w = (np.arange(R) + 1.0) / R
    qb = _blocked(dy * x, L)
    rb.absq = np.abs(qb)
    rb.A, rb.Bq = (qb * w).sum(-1), (qb * (1.0 - w)).sum(-1)
    rb.dG = rb.A.copy()
    if mut != "next_block_dropped":
        rb.dG[:, :-1] += rb.Bq[:, 1:]
    rb.ds = -LN10_20 * G * rb.dG
    att, rg = (tape >> 2) & 1, tape & 3
    a = np.where(att == 1, P.aA, P.aR)
    if mut == "coefficients_swapped":
        a = np.where(att == 1, P.aR, P.aA)
    rb.a = a
    rb.tot, rb.dc, rb.carry_in = np.zeros((B, H)), np.zeros((B, H)), np.zeros((B, H))
    carry = np.zeros(B)
    for j in range(H - 1, -1, -1):
        rb.carry_in[:, j] = carry
        tot = rb.ds[:, j] + carry
        rb.tot[:, j], rb.dc[:, j] = tot, a[:, j] * tot
        carry = tot if mut == "carry_unscaled" else (1.0 - a[:, j]) * tot
    rb.d = 10.0 * np.log10(p + EPS) - P.T
    rb.cp = slope(rb.d, rg, P, mut)
    rb.arg = p + EPS
    rb.dp = rb.dc * rb.cp * C10 / rb.arg * (2.0 / R)
    rb.g = interp(G, P.makeup, L)
    rb.side = np.repeat(rb.dp, R, axis=1)[:, :L] * x
    rb.dx = rb.g * dy if mut == "sidechain_dropped" else rb.g * dy + rb.side
    return rb


# ------------------------------------------------------------------------------------------------------------------ the bound
def bound(x, L, P, r):
    """element-wise bounds on |kernel - model| of the forward for the model run r -> namespace (p, d, c, s, G (B, H); g, y (B, L);
    amb_rg, amb_att (B, H))"""
    x = np.abs(np.asarray(x, f64)[:, :L])
    B, H = r.p.shape
    q = SimpleNamespace()
    q.p = gamma(8) * r.p
    q.arg = q.p + U * EPS + U * (r.arg + q.p)
    rel = q.arg / r.arg
    bl10 = -np.log1p(-rel) / math.log(10.0)
    bl10 = bl10 + 2 * ULP_LOG * U * (np.abs(np.log10(r.arg)) + bl10)
    bl = 10.0 * bl10 + U * (np.abs(r.l) + 10.0 * bl10)
    q.d = bl + U * (np.abs(r.d) + bl)
    q.amb_rg = (np.abs(2.0 * r.d + P.W) <= 2.0 * q.d) | (np.abs(2.0 * r.d - P.W) <= 2.0 * q.d)
    q.c = P.k * q.d + P.kq * (2.0 * q.d) ** 2 + gamma(6) * (np.abs(r.c) + P.k * q.d)
    q.c = np.where((r.rg == 0) & ~q.amb_rg, 0.0, q.c)
    lam, amax = max(1.0 - P.aA, 1.0 - P.aR), max(P.aA, P.aR)
    q.s, q.sprev, q.amb_att = np.zeros((B, H)), np.zeros((B, H)), np.zeros((B, H), bool)
    bs = np.zeros(B)
    for j in range(H):
        q.sprev[:, j] = bs
        gap, room = np.abs(r.c[:, j] - r.sprev[:, j]), q.c[:, j] + bs
        amb = (gap <= room) & (room > 0)
        a = np.where(r.att[:, j], P.aA, P.aR)
        lead = np.where(amb, lam, 1.0 - a) * bs + np.where(amb, amax, a) * q.c[:, j]
        live = (lead > 0) | (r.s[:, j] != 0) | (gap > 0)
        bs = lead + U * (2.0 * amax * (gap + room) + np.abs(r.s[:, j]) + lead) + np.where(live, TINY, 0.0)
        q.s[:, j], q.amb_att[:, j] = bs, amb

    def gain_bound(s, bs):
        t = (P.makeup - s) / 20.0
        bt = bs / 20.0 + gamma(3) * (np.abs(t) + bs / 20.0)
        return 10.0 ** t * (np.expm1(math.log(10.0) * bt) + 2 * ULP_EXP * U * np.exp(math.log(10.0) * bt))
    q.G = gain_bound(r.s, q.s)
    q.G0 = float(gain_bound(np.zeros(1), np.zeros(1))[0])
    G0 = 10.0 ** (P.makeup / 20.0)
    Gp, bGp = np.concatenate([np.full((B, 1), G0), r.G[:, :-1]], 1), np.concatenate([np.full((B, 1), q.G0), q.G[:, :-1]], 1)
    w = (np.arange(R) + 1.0) / R
    bg = (1.0 - w) * bGp[..., None] + w * q.G[..., None] + gamma(3) * (Gp + r.G + bGp + q.G)[..., None]
    q.g = bg.reshape(B, H * R)[:, :L]
    q.y = x * q.g + U * (np.abs(r.y) + x * q.g)
    return q


def bound_bwd(x, dy, L, P, r, q, rb, tape):
    """element-wise bound (B, L) on |kernel - model| of dx, for the model backward rb run with `tape`"""
    x, dy = np.abs(np.asarray(x, f64)[:, :L]), np.abs(np.asarray(dy, f64)[:, :L])
    B, H = r.p.shape
    w = (np.arange(R) + 1.0) / R
    absA, absB = (rb.absq * w).sum(-1), (rb.absq * (1.0 - w)).sum(-1)
    absdG = absA.copy()
    absdG[:, :-1] += absB[:, 1:]
    bdG = gamma(11) * absdG
    inner = q.G * (np.abs(rb.dG) + bdG) + r.G * bdG
    bds = LN10_20 * inner + gamma(3) * (np.abs(rb.ds) + LN10_20 * inner)
    a = rb.a
    bdc = np.zeros((B, H))
    bcarry = np.zeros(B)
    for j in range(H - 1, -1, -1):
        lead = bds[:, j] + bcarry
        btot = lead + U * (np.abs(rb.tot[:, j]) + lead)
        bdc[:, j] = a[:, j] * btot + U * (np.abs(rb.dc[:, j]) + a[:, j] * btot)
        bcarry = (1.0 - a[:, j]) * btot + 2 * U * ((1.0 - a[:, j]) * (np.abs(rb.tot[:, j]) + btot))
    rg = tape & 3
    bcp = np.where(rg == 1, 2.0 * P.kq * q.d + gamma(3) * (np.abs(rb.cp) + 2.0 * P.kq * q.d), 0.0)
    n1 = np.abs(rb.dc * rb.cp)
    bn1 = np.abs(rb.cp) * bdc + np.abs(rb.dc) * bcp + bdc * bcp
    rel = q.arg / r.arg
    scale = C10 / r.arg * (2.0 / R)
    bdp = ((n1 + bn1) / (1.0 - rel) - n1) * scale + gamma(4) * (n1 + bn1) / (1.0 - rel) * scale
    bside = np.repeat(bdp, R, axis=1)[:, :L]
    first, second = dy * q.g, x * bside
    return first + second + gamma(3) * (np.abs(rb.g) * dy + np.abs(rb.side) + first + second)


def tape_differences_allowed(tape, r, q):
    """True when `tape` differs from the model's only in bits the model is ambiguous about"""
    rg_ok = ((tape & 3) == r.rg) | q.amb_rg
    att_ok = (((tape >> 2) & 1) == r.att) | q.amb_att
    return bool(rg_ok.all() and att_ok.all() and ((tape & 0xF8) == 0).all())


def ambiguous_share(q):
    return float((q.amb_rg | q.amb_att).mean())


# ------------------------------------------------------------------------------------------------------------------ fp32 emulation
def _lane_tree(terms):
    """terms (B, H, 64) fp32 -> (B, H): a lane adds its four terms left to right, then the 16 lanes add over distances 1, 2, 4, 8"""
    t = terms.reshape(terms.shape[0], terms.shape[1], 16, 4)
    v = t[..., 0]
    for e in range(1, 4):
        v = v + t[..., e]
    lane = np.arange(16)
    for m in (1, 2, 4, 8):
        v = v + v[..., lane ^ m]
    return v[..., 0]


def _level(p, P):
    return f32(10) * np.log10(p + f32(EPS)) - f32(P.T)


def emulate(x, L, P):
    """fp32 emulation of drc_fwd -> namespace (y (B, L); p, G, s (B, H); tape)"""
    x = np.asarray(x, f32)[:, :L]
    B, H = x.shape[0], blocks(L)
    e = SimpleNamespace()
    xb = _blocked(x, L, f32)
    e.p = _lane_tree(xb * xb) * f32(1.0 / R)
    d = _level(e.p, P)
    W, k, kq = f32(P.W), f32(P.k), f32(P.kq)
    rg = np.where(f32(2) * d < -W, 0, np.where(f32(2) * d <= W, 1, 2))
    t = d + f32(0.5) * W
    c = np.where(rg == 0, f32(0), np.where(rg == 1, kq * t * t, k * d)).astype(f32)
    e.s, att = np.zeros((B, H), f32), np.zeros((B, H), bool)
    s = np.zeros(B, f32)
    for j in range(H):
        att[:, j] = c[:, j] > s
        s = s + np.where(att[:, j], f32(P.aA), f32(P.aR)) * (c[:, j] - s)
        e.s[:, j] = s
    e.G = np.power(f32(10), (f32(P.makeup) - e.s) * f32(0.05))
    e.y = interp(e.G, P.makeup, L, dtype=f32) * x
    e.tape = (rg | (att.astype(np.int64) << 2)).astype(np.uint8)
    assert e.p.dtype == f32 and e.G.dtype == f32 and e.y.dtype == f32 and e.s.dtype == f32
    return e


def emulate_bwd(x, dy, L, P, e):
    """fp32 emulation of drc_bwd on the state and the tape of the emulated forward e -> dx (B, L)"""
    x, dy = np.asarray(x, f32)[:, :L], np.asarray(dy, f32)[:, :L]
    B, H = x.shape[0], blocks(L)
    w = ((np.arange(R) + 1) / R).astype(f32)
    qb = _blocked(dy * x, L, f32)
    A, Bq = _lane_tree(qb * w), _lane_tree(qb * (f32(1) - w))
    dG = A.copy()
    dG[:, :-1] = A[:, :-1] + Bq[:, 1:]
    work = (e.G * dG) * f32(-LN10_20)
    att, rg = (e.tape >> 2) & 1, e.tape & 3
    a = np.where(att == 1, f32(P.aA), f32(P.aR)).astype(f32)
    b = np.where(att == 1, f32(1.0 - P.aA), f32(1.0 - P.aR)).astype(f32)
    dc = np.zeros((B, H), f32)
    carry = np.zeros(B, f32)
    for j in range(H - 1, -1, -1):
        tot = work[:, j] + carry
        dc[:, j] = a[:, j] * tot
        carry = b[:, j] * tot
    cp = np.where(rg == 0, f32(0), np.where(rg == 1, f32(2) * f32(P.kq) * (_level(e.p, P) + f32(0.5) * f32(P.W)), f32(P.k))).astype(f32)
    dp = ((dc * cp) * f32(C10)) / (e.p + f32(EPS)) * f32(2.0 / R)
    dx = interp(e.G, P.makeup, L, dtype=f32) * dy + np.repeat(dp, R, axis=1)[:, :L] * x
    assert dx.dtype == f32
    return dx


# ------------------------------------------------------------------------------------------------------------------ mutants
# name -> (stage: "fwd" judged on y, "bwd" judged on dx with the model's tape; case names).  Every listed case is run; the mutant must leave
# the bound in at least one.
MUTANTS = {
    "sidechain_dropped": ("bwd", ["L6400", "L1000"]),                       # dx = g dy only
    "no_interpolation": ("fwd", ["L6400", "L65"]),                          # G[j-1] taken as G[j]
    "weight_r_over_64": ("fwd", ["L6400", "L1000_hard"]),                   # w_r = r / 64
    "carry_unscaled": ("bwd", ["L6400", "L6400_fastrel"]),                  # carry not multiplied by (1 - a_j)
    "coefficients_swapped": ("bwd", ["L6400", "L6400_fastrel"]),            # aA and aR swapped in the backward
    "next_block_dropped": ("bwd", ["L6400", "L65"]),                        # the next block's (1 - w_r) contribution to dG dropped
    "partial_block_own_mean": ("fwd", ["L1000", "L20037_stride"]),          # the last partial block's mean over its own length
    "state_of_clip_0": ("bwd", ["L6400", "L1000"]),                         # every clip reading clip 0's state
    "knee_slope_above_knee": ("bwd", ["L6400", "L6400_limiter"]),           # c' of region 1 used in region 2
}


_RUNS = {}


def reference(c):
    """(model forward r, forward bounds q, model backward rb with the model's own tape, bound of dx) of a case: computed once, shared, never
    modified"""
    if c.name not in _RUNS:
        i = inputs(c)
        r = model(i.x, c.L, c.P)
        q = bound(i.x, c.L, c.P, r)
        rb = model_bwd(i.x, i.dy, c.L, c.P, r, r.tape)
        _RUNS[c.name] = (r, q, rb, bound_bwd(i.x, i.dy, c.L, c.P, r, q, rb, r.tape))
    return _RUNS[c.name]


def judge_bwd(c, dx, tape):
    """largest |dx - model backward with `tape`| / bound for a backward that used `tape`"""
    i = inputs(c)
    r, q, rb, qdx = reference(c)
    if not np.array_equal(tape, r.tape):
        rb = model_bwd(i.x, i.dy, c.L, c.P, r, tape)
        qdx = bound_bwd(i.x, i.dy, c.L, c.P, r, q, rb, tape)
    return ratio(dx, rb.dx, qdx)


def run_mutant(c, mut, stage):
    """largest |mutated model - model| / bound"""
    i = inputs(c)
    r, q, rb, qdx = reference(c)
    if stage == "fwd":
        return ratio(model(i.x, c.L, c.P, mut).y, r.y, q.y)
    return ratio(model_bwd(i.x, i.dy, c.L, c.P, r, r.tape, mut).dx, rb.dx, qdx)
