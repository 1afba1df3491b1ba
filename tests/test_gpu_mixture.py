"""-m gpu: source separation (diffmusic_amd/inverse_problem/mixture.py, csrc/mix.hip) -- K stems as the batch, mixed under one loss.

Kernel level: `stem_mix_fwd`, `stem_mix_bwd` and `stem_project` bit for bit against their fp32 torch restatements (a loop of separate
multiplies and adds on the CPU), on rows 4 bytes off alignment too; the adjoint identity; the residual after `project`; both bindings; every
refusal.  Operator level: `MixtureOperator.guidance` equals the explicit chain mix -> inner.guidance -> transpose, bit for bit, around
five inner operators.  Step level: teacher-forced steps against `oracle.schedulers` with `per_clip_norm=False` around `OracleMixture`
(below), after the oracle alone has shown that the gains and the coupling matter.  Call level: `pipe(...)` equals a hand-written loop
bit for bit (cold, warm-started, with a NaN restart), a mixture of a track returns (K, T), and a call without a mixture is untouched."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_step import HIFI, VAE, SCHED, H, W as LAT_W, LEN               # noqa: E402
from tests.test_gpu_track import OracleTrack, T3, R3, _FixedNoiser                   # noqa: E402

EPS32 = 2.0 ** -23
K3, GAINS = 3, (2.0, 0.25, 1.0)


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-300))


def _dot(a, b):
    return float((a.double().cpu().reshape(-1) * b.double().cpu().reshape(-1)).sum())


def _bits(t):
    return t.contiguous().cpu().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _gains(K, base=GAINS):
    """`base` padded (cyclically) or cut to K values."""
    return [base[k % len(base)] for k in range(K)]


# ---- the fp32 restatements (CPU: one rounding per multiply and per add, nothing fused) -------------------------------------------------
def ref_mix(x, gains, K, G, L):
    xs = x[:, :L].cpu().reshape(K, G, L)
    g = torch.tensor([1.0] * K if gains is None else gains, dtype=torch.float32)
    acc = g[0] * xs[0]                                                               # the first term is taken as it is
    for k in range(1, K):
        acc = acc + g[k] * xs[k]
    return acc


def ref_mix_bwd(dmix, gains, K, full):
    G, L = dmix.shape
    g = torch.tensor([1.0] * K if gains is None else gains, dtype=torch.float32)
    out = torch.zeros(K * G, full, dtype=torch.float32)
    for k in range(K):
        out[k * G:(k + 1) * G, :L] = g[k] * dmix.cpu()
    return out


def ref_coeffs(gains, K):
    g = torch.tensor([1.0] * K if gains is None else gains, dtype=torch.float32).double()      # the fp32 gains, then float64
    return (g / (g * g).sum()).float()


def ref_project(x, y, gains, K, L):
    c = ref_coeffs(gains, K)
    r = y.cpu().reshape(1, L) - ref_mix(x, gains, K, 1, L)
    return torch.stack([x[k, :L].cpu() + c[k] * r[0] for k in range(K)])


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------
KERNEL_CASES = [(3, 1, 6400, 32), (3, 1, 6397, 37), (2, 3, 6400, 32), (16, 1, 1027, 5), (1, 1, 6400, 32)]
_IDS = [f"K{c[0]}-G{c[1]}-L{c[2]}-pad{c[3]}" for c in KERNEL_CASES]


def _stems(rows, full, seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.arange(full, dtype=torch.float32)
    x = torch.stack([0.4 * torch.sin(n * (0.01 + 0.003 * r) + r) for r in range(rows)]) + 0.1 * torch.randn(rows, full, generator=g)
    x[0, 5] = -0.0                                                                   # a signed zero must survive K = 1, g = 1
    return x.cuda()


@pytest.mark.parametrize("K,G,L,pad", KERNEL_CASES, ids=_IDS)
def test_mix_forward_is_the_fp32_loop_bit_for_bit(K, G, L, pad):
    from diffmusic_amd import ops
    wav = _stems(K * G, L + pad, 1)
    for x in (wav, wav[:, 1:]):                                                      # the second: rows 4 bytes off 16-byte alignment
        for gains in (_gains(K), None):
            got = ops.hip.stem_mix_fwd(x, gains, K, G, L)
            assert got.shape == (G, L) and got.dtype == torch.float32 and got.is_contiguous()
            assert _same_bits(got, ref_mix(x, gains, K, G, L)), (K, G, L, gains)
        assert _same_bits(ops.hip.stem_mix_fwd(x, None, K, G, L), ops.hip.stem_mix_fwd(x, [1.0] * K, K, G, L))
    if K == 1:                                                                       # g = 1: a copy, -0.0f and NaN included
        wav[0, 7] = float("nan")
        got = ops.hip.stem_mix_fwd(wav, None, 1, 1, L)
        assert _same_bits(got, wav[:, :L]) and int(_bits(got)[0, 5]) == -2 ** 31 and bool(torch.isnan(got[0, 7]))


@pytest.mark.parametrize("K,G,L,pad", KERNEL_CASES, ids=_IDS)
def test_mix_transpose_bits_zero_tail_and_adjoint(K, G, L, pad):
    from diffmusic_amd import ops
    g = torch.Generator().manual_seed(7)
    x = torch.randn(K * G, L + pad, generator=g).cuda()
    d = torch.randn(G, L, generator=g).cuda()
    for full in (L + pad, L + pad - 1, L):
        for gains in (_gains(K), None):
            junk = torch.full((K * G, full), float("nan"), device="cuda")              # the allocator hands this block to the op's output:
            del junk                                                                 # the kernel writes the tail past L itself
            got = ops.hip.stem_mix_bwd(d, gains, K, full)
            assert got.shape == (K * G, full)
            assert _same_bits(got, ref_mix_bwd(d, gains, K, full)), (K, G, L, full, gains)
            assert bool((_bits(got[:, L:]) == 0).all())                              # +0.0f exactly, whatever the gain's sign
        assert _same_bits(ops.hip.stem_mix_bwd(d, None, K, full), ops.hip.stem_mix_bwd(d, [1.0] * K, K, full))
    neg = ops.hip.stem_mix_bwd(d, [-g_ for g_ in _gains(K)], K, L + pad)
    assert bool((_bits(neg[:, L:]) == 0).all())
    gains = _gains(K)
    lhs = _dot(ops.hip.stem_mix_fwd(x, gains, K, G, L), d)
    rhs = _dot(x[:, :L], ops.hip.stem_mix_bwd(d, gains, K, L + pad)[:, :L])
    print(f"\n  <M x, d> = {lhs:.6f}, <x, M^T d> = {rhs:.6f}")
    assert abs(lhs - rhs) <= 2e-4 * max(abs(lhs), abs(rhs), math.sqrt(x[:, :L].numel())), (lhs, rhs)      # the stitch's bound


@pytest.mark.parametrize("K,G,L,pad", [c for c in KERNEL_CASES if c[1] == 1], ids=[i for c, i in zip(KERNEL_CASES, _IDS) if c[1] == 1])
def test_project_bits_and_residual(K, G, L, pad):
    """Bits against the restatement, then max |y - mix(p)| <= 4 * 2^-23 * max(|y|, max_k |g_k p_k|), the residual in float64 from the fp32
    stems.  The residual is that of the definition itself (r carries the roundings of an fp32 sum of K terms), so it grows with K: on these
    inputs the restatement measures 1.3 .. 2.4 of those ulps at K = 3 and 3.0 (gains (2, 0.25, 1) repeated) / 3.7 (unit gains) at K = 16.
    The gains are the ones every kernel test runs with, plus (1, 0.5, 1.5) at K = 3."""
    from diffmusic_amd import ops
    g = torch.Generator().manual_seed(11)
    wav = torch.randn(K, L + pad, generator=g).cuda()
    y = torch.randn(1, L, generator=g).cuda()
    for x in (wav, wav[:, 1:]):
        for gains in [_gains(K), None] + ([[1.0, 0.5, 1.5]] if K == 3 else []):
            p = ops.hip.stem_project(x, y, gains, L)
            assert p.shape == (K, L) and _same_bits(p, ref_project(x, y, gains, K, L)), (K, L, gains)
            gd = torch.tensor([1.0] * K if gains is None else gains, dtype=torch.float64)
            terms = gd[:, None] * p.double().cpu()
            res = float((y.double().cpu()[0] - terms.sum(dim=0)).abs().max())
            scale = max(float(y.abs().max()), float(terms.abs().max()))
            print(f"\n  project K={K} L={L} gains={gains and gains[:3]}: max |y - mix(p)| = {res / (EPS32 * scale):.2f} ulp of the largest term")
            assert res <= 4 * EPS32 * scale, (res, scale)
        assert _same_bits(ops.hip.stem_project(x, y, None, L), ops.hip.stem_project(x, y, [1.0] * K, L))


def test_both_bindings_are_bit_identical():
    from diffmusic_amd import ops
    h = ops.load()
    for K, G, L, pad in KERNEL_CASES:
        wav = _stems(K * G, L + pad, 3)
        d = torch.randn(G, L, generator=torch.Generator().manual_seed(4)).cuda()
        for gains in (_gains(K), None):
            a, b = h.stem_mix_fwd(wav[:, 1:], gains, K, G, L), ops.ctypes_hip.stem_mix_fwd(wav[:, 1:], gains, K, G, L)
            assert _same_bits(a, b) and a.shape == (G, L)
            a, b = h.stem_mix_bwd(d, gains, K, L + pad), ops.ctypes_hip.stem_mix_bwd(d, gains, K, L + pad)
            assert _same_bits(a, b) and a.shape == (K * G, L + pad)
            if G == 1:
                a, b = h.stem_project(wav, d, gains, L), ops.ctypes_hip.stem_project(wav, d, gains, L)
                assert _same_bits(a, b) and a.shape == (K, L)


def test_every_refusal_raises_from_both_bindings_without_a_launch():
    from diffmusic_amd import ops
    h = ops.load()
    L = 64
    wav, d, y = torch.zeros(3, L + 8).cuda(), torch.zeros(1, L).cuda(), torch.zeros(1, L).cuda()
    many = torch.zeros(17, L).cuda()
    nan, inf = float("nan"), float("inf")
    for b in (h, ops.ctypes_hip):
        with pytest.raises(RuntimeError, match="1 <= stems <= 16"):
            b.stem_mix_fwd(many, None, 17, 1, L)
        with pytest.raises(RuntimeError, match="1 <= stems <= 16"):
            b.stem_mix_fwd(many[:0], None, 0, 1, L)
        with pytest.raises(RuntimeError, match="1 <= stems <= 16"):
            b.stem_mix_bwd(d, None, 17, L)
        with pytest.raises(RuntimeError, match="1 <= stems <= 16"):
            b.stem_mix_bwd(d, None, 0, L)
        with pytest.raises(RuntimeError, match="1 <= stems <= 16"):
            b.stem_project(many, y, None, L)
        with pytest.raises(RuntimeError, match="groups >= 1 and L >= 1"):
            b.stem_mix_fwd(wav[:0], None, 3, 0, L)
        with pytest.raises(RuntimeError, match="groups >= 1 and L >= 1"):
            b.stem_mix_fwd(wav, None, 3, 1, 0)
        with pytest.raises(RuntimeError, match="groups >= 1 and L >= 1"):
            b.stem_mix_bwd(d[:, :0], None, 3, L)
        with pytest.raises(RuntimeError, match="L >= 1"):
            b.stem_project(wav, y[:, :0], None, 0)
        with pytest.raises(RuntimeError, match="row stride >= L"):
            b.stem_mix_fwd(wav.as_strided((3, L), (L - 1, 1)), None, 3, 1, L)
        with pytest.raises(RuntimeError, match="row stride >= L"):
            b.stem_project(wav.as_strided((3, L), (L - 1, 1)), y, None, L)
        with pytest.raises(RuntimeError, match="full >= L"):
            b.stem_mix_bwd(d, None, 3, L - 1)
        for bad in (nan, inf, -inf, 1e39):
            with pytest.raises(RuntimeError, match="not finite"):
                b.stem_mix_fwd(wav, [1.0, bad, 1.0], 3, 1, L)
            with pytest.raises(RuntimeError, match="not finite"):
                b.stem_mix_bwd(d, [1.0, bad, 1.0], 3, L)
            with pytest.raises(RuntimeError, match="not finite"):
                b.stem_project(wav, y, [bad, 1.0, 1.0], L)
        with pytest.raises(RuntimeError, match="no finite correction"):
            b.stem_project(wav, y, [0.0, 0.0, 0.0], L)
        with pytest.raises(RuntimeError, match="grid out of range"):
            b.stem_mix_fwd(torch.zeros(65536, 1).cuda(), None, 1, 65536, 1)
        with pytest.raises(RuntimeError, match="grid out of range"):
            b.stem_mix_bwd(torch.zeros(65536, 1).cuda(), None, 1, 1)
        with pytest.raises(RuntimeError, match="2 gains for 3 stems"):
            b.stem_mix_fwd(wav, [1.0, 1.0], 3, 1, L)
        with pytest.raises(RuntimeError, match="expected \\(6, >= 64\\)"):
            b.stem_mix_fwd(wav, None, 3, 2, L)                                         # fewer rows than K * G: never launched
    torch.cuda.synchronize()


# ---- operator level -------------------------------------------------------------------------------------------------------------------
def _inner(kind):
    """(inner operator, G, clean (1, T) signal -> measurement keywords)."""
    from diffmusic_amd import inverse_problem as P
    n = P.get_noiser("gaussian", 0.0)
    if kind == "identity":
        return P.IdentityOperator(16000), None
    if kind == "inpainting":
        return P.MusicInpaintingOperator(1, LEN, "box", 0.25, 0.5, 0.3, 0.1, 0.2, noiser=n), None
    if kind == "declipping":
        return P.DeclippingOperator(16000, 0.3, noiser=n), None
    if kind == "dereverberation":
        return P.MusicDereverberationOperator(500, 0.99, noiser=n, fixed_ir=True), None
    assert kind == "track_identity"
    lay = P.TrackLayout(T3, LEN, R3)
    return P.TrackOperator(P.IdentityOperator(16000), lay), lay


@pytest.mark.parametrize("kind", ["identity", "inpainting", "declipping", "dereverberation", "track_identity"])
def test_guidance_is_the_explicit_chain_bit_for_bit(kind):
    from diffmusic_amd import inverse_problem as P, ops
    inner, lay = _inner(kind)
    G = 1 if lay is None else lay.num_windows
    T = LEN if lay is None else lay.track_len
    op = P.MixtureOperator(inner, K3, GAINS)
    assert op.groups == G and op.num_clips == K3 * G
    g = torch.Generator().manual_seed(5)
    clean = (0.3 * torch.sin(torch.arange(T) * 0.05)[None] * torch.tensor([[1.0], [0.6], [0.8]]) + 0.05 * torch.randn(K3, T, generator=g)).cuda()
    y = op.forward(clean)
    assert y.shape[0] == 1
    wav = (0.2 * torch.randn(K3 * G, LEN + 32, generator=g)).cuda()
    assert op.dead_span(LEN) == (inner.dead_span(LEN) if lay is None else None)
    if kind == "inpainting":
        assert op.dead_span(LEN) == (1600, 3200)
    for space in ("mel_spectrogram", "wav_form"):
        loss, dwav = op.guidance(wav, LEN, y, space)
        mix = ops.hip.stem_mix_fwd(wav, list(GAINS), K3, G, LEN)
        l0, dmix = inner.guidance(mix, LEN, y, space)
        want = ops.hip.stem_mix_bwd(dmix.contiguous(), list(GAINS), K3, LEN + 32)
        assert loss.shape == (1,) and dwav.shape == (K3 * G, LEN + 32)
        assert torch.equal(loss, l0) and _same_bits(dwav, want), (kind, space)
        assert all(float(dwav[r].abs().max()) > 0 for r in range(K3 * G)) and bool(torch.isfinite(dwav).all())
    # forward is the inner operator on the mix of the stems
    assert _same_bits(y, inner.forward(ops.hip.stem_mix_fwd(clean, list(GAINS), K3, 1, T)))


@pytest.mark.parametrize("kind", ["identity", "inpainting", "declipping", "dereverberation"])
def test_one_stem_unit_gain_equals_the_inner_operator_bit_for_bit(kind):
    from diffmusic_amd import inverse_problem as P
    inner, _ = _inner(kind)
    g = torch.Generator().manual_seed(6)
    clean = (0.3 * torch.sin(torch.arange(LEN) * 0.05)[None] + 0.05 * torch.randn(1, LEN, generator=g)).cuda()
    wav = (0.2 * torch.randn(1, LEN + 32, generator=g)).cuda()
    for gains in (None, [1.0]):
        op = P.MixtureOperator(inner, 1, gains)
        y = inner.forward(clean)
        assert _same_bits(op.forward(clean), y)
        for space in ("mel_spectrogram", "wav_form"):
            l0, d0 = inner.guidance(wav, LEN, y, space)
            l1, d1 = op.guidance(wav, LEN, y, space)
            assert torch.equal(l0, l1) and _same_bits(d0, d1), (kind, space)


def test_project_stage():
    from diffmusic_amd import inverse_problem as P
    op = P.MixtureOperator(P.IdentityOperator(16000), K3, GAINS)
    g = torch.Generator().manual_seed(8)
    stems, y = torch.randn(K3, LEN + 32, generator=g), torch.randn(1, LEN, generator=g).cuda()
    p = op.project(stems.numpy(), y)                                                 # what `pipe(...).audios` hands over: a host array
    assert _same_bits(p, ref_project(stems, y, list(GAINS), K3, LEN))
    with pytest.raises(ValueError, match="not the mixture itself"):
        P.MixtureOperator(_inner("inpainting")[0], K3).project(stems, y)


# ---- step level -----------------------------------------------------------------------------------------------------------------------
class OracleMixture:
    """The oracle-side MixtureOperator: `forward` sums g_k * wav_k in torch (differentiable; rows stem-major, G groups) and calls the
    oracle operator -- or `OracleTrack` -- on the (G, L) mixtures."""

    def __init__(self, inner, gains, groups=1):
        self.inner, self.gains, self.groups = inner, [float(g) for g in gains], groups

    def mix(self, wav):
        K, G = len(self.gains), self.groups
        xs = wav.reshape(K, G, wav.shape[-1])
        return sum(self.gains[k] * xs[k] for k in range(K))

    def forward(self, wav, **k):
        return self.inner.forward(self.mix(wav), **k)

    def transform(self, x):
        return self.inner.transform(x)

    def inverse_transform(self, mel, vocoder):
        return self.inner.inverse_transform(mel, vocoder)


@pytest.fixture(scope="module")
def nets():
    from diffmusic_amd.engine import HifiGanEngine, VaeDecoderEngine
    from oracle.models import HifiGan, VaeDecoder
    voc, vae = HifiGanEngine(HIFI), VaeDecoderEngine(VAE)
    sv, sa = voc.synth_state_dict(seed=1), vae.synth_state_dict(seed=2)
    voc.load_state_dict(sv)
    vae.load_state_dict(sa)
    rvoc, rvae = HifiGan(**HIFI), VaeDecoder(**VAE)
    rvoc.load_state_dict(sv, strict=False)
    rvae.load_state_dict(sa, strict=True)
    return voc, vae, rvoc.eval(), rvae.eval()


def _step_ops(task, T, sigma=0.0):
    """(product operator, oracle operator), both built for a signal of T samples."""
    from diffmusic_amd import inverse_problem as P
    from oracle import operators as O
    n, rn = P.get_noiser("gaussian", sigma), O.get_noiser("gaussian", 0.0)
    if task == "identity":
        return P.IdentityOperator(16000), O.IdentityOperator(16000)
    if task == "music_inpainting":
        args = (1, T, "box", 0.28, 0.42, 0.3, 0.1, 0.2)
        return P.MusicInpaintingOperator(*args, noiser=n), O.MusicInpaintingOperator(*args, noiser=rn)
    assert task == "music_dereverberation"
    return P.MusicDereverberationOperator(500, 0.99, noiser=n), O.MusicDereverberationOperator(500, 0.99, noiser=rn)


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.double().cpu().flatten(), b.double().cpu().flatten(), dim=0).item()


STEP_CASES = [("dps", "identity", 0.0, 5e-4, "mel_spectrogram", 501, 0.0, False),
              ("dps", "identity", 0.0, 5e-4, "wav_form", 996, 0.0, False),
              ("dps", "music_inpainting", 0.0, 5e-4, "mel_spectrogram", 501, 0.0, False),
              ("mpgd", "music_dereverberation", 0.0, 5e-3, "mel_spectrogram", 501, 0.0, False),
              ("dsg", "identity", 1.0, 0.08, "mel_spectrogram", 501, 0.0, False),
              ("dps", "music_inpainting", 0.0, 5e-4, "mel_spectrogram", 501, 0.05, False),
              ("dps", "music_inpainting", 0.0, 5e-4, "mel_spectrogram", 501, 0.0, True)]


@pytest.mark.parametrize("name,task,eta,rate,space,t,sigma,track", STEP_CASES,
                         ids=[f"{c[0]}-{c[1]}-{c[4]}-sigma{c[6]}{'-track' if c[7] else ''}" for c in STEP_CASES])
def test_teacher_forced_mixture_step(nets, name, task, eta, rate, space, t, sigma, track):
    """`_teacher_forced` of tests/test_gpu_step.py on K = 3 stems with gains (2, 0.25, 1): same x, eps and noise on both sides, its
    bounds (loss < 1e-2, prev_sample rel-L2 < 1e-2, gradient cosine over the whole (K, ...) tensor > 0.98).  Before that, on the oracle
    alone: the gradient with the gains is less than 0.9 in cosine from the gradient with unit gains and with the gains reversed (the
    loss at random weights hardly sees the gains, the gradient does), and for the identity the mixture's loss is more than 2e-2 from the
    whole-batch norm of the stems each scored against y -- so a product that dropped the gains, their order or the coupling cannot pass."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    from oracle import schedulers as OS
    voc, vae, rvoc, rvae = nets
    lay = P.TrackLayout(T3, LEN, R3) if track else None
    G = 1 if lay is None else lay.num_windows
    T = LEN if lay is None else T3
    B = K3 * G
    op, rop = _step_ops(task, T, sigma)
    g = torch.Generator().manual_seed(77)
    clean = 0.3 * torch.sin(torch.arange(T) * 0.05)[None] * torch.tensor([[1.0], [0.6], [0.8]]) + 0.05 * torch.randn(K3, T, generator=g)
    opk = dict(ir=rop.generate_impulse_response(500, 0.99)) if task == "music_dereverberation" else {}
    x = torch.randn(B, 8, H, LAT_W, generator=g)
    e = torch.randn(B, 8, H, LAT_W, generator=g)
    z = torch.randn(B, 8, H, LAT_W, generator=g)

    def oracle_op(gains):
        return OracleMixture(rop if lay is None else OracleTrack(rop, lay), gains, G)
    top = P.MixtureOperator(op if lay is None else P.TrackOperator(op, lay), K3, GAINS)
    y_ref = rop.forward(OracleMixture(rop, GAINS).mix(clean), **opk)                 # (K, T) stems -> the (1, T) mixture -> A
    assert y_ref.shape[0] == 1
    z_step = None
    if sigma > 0:
        z_meas, z_step = torch.randn(y_ref.shape, generator=g), torch.randn(y_ref.shape, generator=g)
        y_ref = y_ref + sigma * z_meas                                              # the measurement's own draw, made once
        y = y_ref.cuda()
        rop.noiser = _FixedNoiser(sigma, z_step)
    else:
        y = top.forward(clean.cuda(), **opk)
        assert _rel(y, y_ref) < 1e-4, "MixtureOperator.forward"
    kw = dict(eta=eta, ip_guidance_rate=rate, original_waveform_length=LEN, supervised_space=space)
    rnoise = dict(sample_noise=z) if name in ("dsg", "diffmusic") else dict(variance_noise=z if eta > 0 else None)

    def oracle_step(gains):
        rs = OS.get_scheduler(name)(operator=oracle_op(gains), per_clip_norm=False, **SCHED)
        rs.set_timesteps(200)
        return rs, rs.step(e, t, x, measurement=y_ref, vae=rvae, vocoder=rvoc, op_kwargs=opk, **kw, **rnoise)
    rs, ro = oracle_step(GAINS)
    assert ro.loss.numel() == 1
    # the discriminating conditions, on the oracle alone
    c_unit, c_rev = _cos(ro.sample, oracle_step((1.0, 1.0, 1.0))[1].sample), _cos(ro.sample, oracle_step(GAINS[::-1])[1].sample)
    print(f"\n  {name}/{task}/{space}: oracle gradient vs unit gains cos {c_unit:.3f}, vs reversed gains cos {c_rev:.3f}")
    assert c_unit < 0.9 and c_rev < 0.9, (c_unit, c_rev)
    if task == "identity" and name == "dps":
        a_t = float(rs.alphas_cumprod[t])
        with torch.no_grad():
            wav = rop.inverse_transform(rvae.decode((x - (1 - a_t) ** 0.5 * e) / a_t ** 0.5 / rvae.config.scaling_factor).sample, rvoc)[:, :LEN]
            tf = rop.transform if space == "mel_spectrogram" else (lambda v: v)
            whole = float(torch.linalg.norm(tf(y_ref) - tf(OracleMixture(rop, GAINS).mix(wav))))
            separate = float(torch.linalg.norm(torch.stack([torch.linalg.norm(tf(y_ref) - tf(wav[k:k + 1])) for k in range(K3)])))
        gap = abs(whole - separate) / whole
        print(f"  oracle loss of the mixture {whole:.4f}, of the stems scored separately {separate:.4f}: {gap:.3f} apart")
        assert gap > 2e-2, (whole, separate)
    sched = get_scheduler(name)(operator=top, per_clip_norm=False, **SCHED)
    sched.set_timesteps(200)
    sched.debug_keep_grad = True
    noise_kw = dict(sample_noise=z.cuda()) if name in ("dsg", "diffmusic") else dict(variance_noise=z.cuda() if eta > 0 else None)
    popk = dict(opk, noise=z_step.cuda()) if sigma > 0 else opk
    out = sched.step(e.cuda(), t, x.cuda(), measurement=y, vae=vae, vocoder=voc, op_kwargs=popk, **kw, **noise_kw)
    torch.cuda.synchronize()
    assert out.loss.numel() == 1 and out.prev_sample.shape == x.shape
    rp, rl = _rel(out.prev_sample, ro.prev_sample), _rel(out.loss.reshape(-1), ro.loss.reshape(-1))
    cos = _cos(sched.last_grad, ro.sample)
    msg = f"mixture {name}/{task}/{space}/sigma={sigma}/track={track}: prev {rp:.2e} loss {rl:.2e} grad {_rel(sched.last_grad, ro.sample):.2e} cos {cos:.4f}"
    print("  " + msg)
    assert _rel(out.pred_original_sample, ro.pred_original_sample) < 1e-4 or name == "mpgd"
    assert rl < 1e-2, msg
    assert cos > 0.98, msg
    assert rp < 1e-2, msg
    assert all(float(sched.last_grad[r].abs().max()) > 0 for r in range(B)), "the gradient reaches every stem"


def test_per_clip_norm_scheduler_is_refused_at_step(nets):
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    voc, vae, _, _ = nets
    sched = get_scheduler("dps")(operator=P.MixtureOperator(P.IdentityOperator(16000), K3, GAINS), **SCHED)
    sched.set_timesteps(200)
    x = torch.randn(K3, 8, H, LAT_W).cuda()
    with pytest.raises(ValueError, match="MixtureOperator makes the batch one sample.*per_clip_norm=False"):
        sched.step(x, 501, x, measurement=torch.zeros(1, LEN).cuda(), vae=vae, vocoder=voc, original_waveform_length=LEN)


# ---- call level -----------------------------------------------------------------------------------------------------------------------
N_CALL, SECONDS = 4, 0.4


def _pipe(operator, per_clip_norm=False):
    from diffmusic_amd.pipelines import get_pipeline
    from diffmusic_amd.schedulers import get_scheduler
    from tests.test_gpu_warm_start import HIFI as HIFI_SR, UNET
    pipe = get_pipeline("musicldm").from_pretrained("synthetic", seed=0, unet_config=UNET, vae_config=VAE, vocoder_config=HIFI_SR).to("cuda")
    pipe.scheduler = get_scheduler("dps")(operator=operator, per_clip_norm=per_clip_norm, **SCHED)
    pipe.assume_uncond_equals_cond = True
    return pipe


def _mixture_pipe(track=False):
    from diffmusic_amd import inverse_problem as P
    lay = P.TrackLayout(T3, LEN, R3) if track else None
    T = T3 if track else LEN
    inner = P.MusicInpaintingOperator(1, T, "box", 0.28, 0.42, 0.3, 0.1, 0.2, noiser=P.get_noiser("gaussian", 0.0))
    op = P.MixtureOperator(inner if lay is None else P.TrackOperator(inner, lay), K3, GAINS)
    return _pipe(op), op, lay


def _inputs(B, T, seed=21):
    g = torch.Generator().manual_seed(seed)
    clean = 0.3 * torch.sin(torch.arange(T) * 0.05)[None] * torch.tensor([[1.0], [0.6], [0.8]]) + 0.05 * torch.randn(K3, T, generator=g)
    return clean, torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)


def _gens(B):
    return [torch.Generator().manual_seed(300 + k) for k in range(B)]


def _hand_loop(pipe, pe, y, B, timesteps=None, start=None):
    """`_unet_eps` + `scheduler.step` + decode, written out; returns (vocoder output (B, full), latents, losses)."""
    dev = torch.device("cuda")
    s = pipe.scheduler
    if start is None:
        gens = _gens(B)
        s.set_timesteps(N_CALL, device="cuda")
        timesteps = list(s._timesteps_host)
        x = pipe.prepare_latents(B, 8, 40, torch.float32, dev, gens, None)
    else:
        x, gens = start
    c = pipe._prepare_cond(pe, None, 1, True, dev)
    losses = []
    for t in timesteps:
        eps = pipe._unet_eps(x, t, c, pipe.default_guidance_scale, True)
        o = s.step(eps, t, x, eta=0.0, generator=gens, measurement=y, vae=pipe.vae, vocoder=pipe.vocoder, original_waveform_length=LEN,
                   ip_guidance_rate=5e-4, supervised_space="mel_spectrogram")
        x = o.prev_sample
        losses.append(o.loss)
    wav = pipe.vocoder(pipe.vae.decode(x / pipe.vae.config.scaling_factor).sample.squeeze(1)).float()
    return wav, x, losses


def test_mixture_call_equals_the_hand_written_loop():
    pipe, op, _ = _mixture_pipe()
    clean, pe = _inputs(K3, LEN)
    y = op.forward(clean.cuda())
    call = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0)
    out = pipe(generator=_gens(K3), output_type="pt", **call).audios
    assert out.shape == (K3, LEN) and pipe.nan_restarts == 0
    assert len(pipe.last_losses) == N_CALL and all(l.numel() == 1 for l in pipe.last_losses)      # one loss for the whole mixture
    got_losses = list(pipe.last_losses)
    lat = pipe(generator=_gens(K3), output_type="latent", **call).audios
    assert lat.shape == (K3, 8, 10, 16)
    wav, x, losses = _hand_loop(pipe, pe, y, K3)
    assert torch.equal(lat, x) and torch.equal(out, wav[:, :LEN].cpu())
    assert all(torch.equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(got_losses, losses))
    assert out.abs().max() > 0 and bool(torch.isfinite(out).all())


def test_warm_started_mixture_call_equals_its_hand_loop():
    """`init_audio` = y / K for every stem, `strength=0.5`: 2 of 4 steps, from the encoded share of the mixture."""
    from diffmusic_amd.torch_utils import randn_tensor
    pipe, op, _ = _mixture_pipe()
    clean, pe = _inputs(K3, LEN)
    y = op.forward(clean.cuda())
    init = (y / K3).repeat(K3, 1)
    out = pipe(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0,
               generator=_gens(K3), output_type="pt", init_audio=init, strength=0.5).audios
    assert len(pipe.last_losses) == 2 and out.shape == (K3, LEN)
    s = pipe.scheduler
    s.set_timesteps(N_CALL, device="cuda")
    ts = s.timesteps_for_strength(0.5)
    assert ts == list(s._timesteps_host)[2:]
    gens, dev = _gens(K3), torch.device("cuda")
    z0 = pipe._encode_init(init, True, "sample", gens, LEN, 40, dev)
    x = s.add_noise(z0, randn_tensor(z0.shape, generator=gens, device=dev, dtype=torch.float32), ts[0])
    wav, _, _ = _hand_loop(pipe, pe, y, K3, timesteps=ts, start=(x, gens))
    assert torch.equal(out, wav[:, :LEN].cpu())


def test_nan_restarts_all_stems():
    pipe, op, _ = _mixture_pipe()
    clean, pe = _inputs(K3, LEN)
    y = op.forward(clean.cuda())
    real_step = pipe.scheduler.step
    state = dict(calls=0, first=[])

    def step(model_output, timestep, sample, **kw):
        out = real_step(model_output, timestep, sample, **kw)
        if timestep == pipe.scheduler._timesteps_host[0]:
            state["first"].append(sample.clone())
        if state["calls"] == 2:
            out.loss = out.loss * float("nan")
        state["calls"] += 1
        return out
    pipe.scheduler.step = step
    gens = _gens(K3)
    out = pipe(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0,
               generator=gens, output_type="pt").audios
    assert pipe.nan_restarts == 1 and state["calls"] == 3 + N_CALL
    a, b = state["first"]
    assert bool((a != b).flatten(1).any(dim=1).all())                                # every stem's latent was redrawn
    # the restarted trajectory is the hand-written loop from the redrawn latents (generators already advanced by the first draw)
    pipe.scheduler.step = real_step
    hg = _gens(K3)
    pipe.prepare_latents(K3, 8, 40, torch.float32, torch.device("cuda"), hg, None)
    pipe.scheduler.set_timesteps(N_CALL, device="cuda")
    x = pipe.prepare_latents(K3, 8, 40, torch.float32, torch.device("cuda"), hg, None)
    assert torch.equal(x, b)
    wav, _, _ = _hand_loop(pipe, pe, y, K3, timesteps=list(pipe.scheduler._timesteps_host), start=(x, hg))
    assert torch.equal(out, wav[:, :LEN].cpu())


def test_mixture_of_a_track_returns_every_stem_stitched():
    pipe, op, lay = _mixture_pipe(track=True)
    Wn = lay.num_windows
    B = K3 * Wn
    clean, pe = _inputs(B, T3)
    y = op.forward(clean.cuda())
    assert y.shape == (1, T3)
    call = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0)
    out = pipe(generator=_gens(B), output_type="pt", **call).audios
    assert out.shape == (K3, T3) and all(l.numel() == 1 for l in pipe.last_losses)
    assert pipe(generator=_gens(B), output_type="latent", **call).audios.shape == (B, 8, 10, 16)
    wav, _, _ = _hand_loop(pipe, pe, y, B)
    want = torch.cat([op.track.stitch(wav[k * Wn:(k + 1) * Wn]) for k in range(K3)])   # stem k owns rows k W .. k W + W - 1
    assert torch.equal(out, want.cpu()) and bool(torch.isfinite(out).all())


def test_call_refusals():
    from diffmusic_amd import inverse_problem as P
    pipe, op, _ = _mixture_pipe()
    clean, pe = _inputs(K3, LEN)
    y = op.forward(clean.cuda())
    call = dict(audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0)
    with pytest.raises(ValueError, match="holds 2 clips, but the mixture has 3 stems"):
        pipe(prompt_embeds=pe[:2], generator=_gens(2), **call)
    with pytest.raises(ValueError, match="source separation cannot be sharded"):
        pipe(prompt_embeds=pe, generator=_gens(K3), shard=True, **call)
    with pytest.raises(ValueError, match="source separation cannot be sharded"):
        pipe(prompt_embeds=pe, generator=_gens(K3), group=object(), **call)
    with pytest.raises(ValueError, match="source separation cannot run as clip lanes"):
        pipe(prompt_embeds=pe, generator=_gens(K3), lanes=2, **call)
    pipe.scheduler.per_clip_norm = True
    with pytest.raises(ValueError, match="source separation needs whole-batch norms"):
        pipe(prompt_embeds=pe, generator=_gens(K3), **call)
    pipe.scheduler.per_clip_norm = False
    op.inner.noiser = P.GaussianNoise(0.05, stream="clip")
    with pytest.raises(ValueError, match="global noise stream"):
        pipe(prompt_embeds=pe, generator=_gens(K3), **call)
    tpipe, top, lay = _mixture_pipe(track=True)
    with pytest.raises(ValueError, match="holds 3 clips, but the mixture has 3 stems of 3 windows"):
        tpipe(prompt_embeds=pe, generator=_gens(K3), **dict(call, measurement=torch.zeros(1, T3).cuda()))


def test_a_call_without_a_mixture_is_untouched(monkeypatch):
    """A plain operator, per-clip norms, B = 3: the call equals a loop written with nothing of the new module, bit for bit, and none of
    the new ops is resolved."""
    from diffmusic_amd import inverse_problem as P, ops
    touched = []
    for name in ("stem_mix_fwd", "stem_mix_bwd", "stem_project"):
        monkeypatch.setattr(ops.ctypes_hip, name, lambda *a, _n=name, **k: touched.append(_n))
    monkeypatch.setattr(P.MixtureOperator, "__init__", lambda self, *a, **k: touched.append("MixtureOperator"))
    real = type(ops.hip).__getattr__
    monkeypatch.setattr(type(ops.hip), "__getattr__", lambda self, n: touched.append(n) if n.startswith("stem_") else real(self, n))
    inner = P.MusicInpaintingOperator(1, LEN, "box", 0.28, 0.42, 0.3, 0.1, 0.2, noiser=P.get_noiser("gaussian", 0.0))
    pipe = _pipe(inner, per_clip_norm=True)
    clean, pe = _inputs(K3, LEN)
    y = inner.forward(clean.cuda())
    out = pipe(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0,
               generator=_gens(K3), output_type="pt").audios
    assert out.shape == (K3, LEN) and all(l.numel() == K3 for l in pipe.last_losses)
    wav, _, _ = _hand_loop(pipe, pe, y, K3)
    assert torch.equal(out, wav[:, :LEN].cpu())
    assert touched == []
