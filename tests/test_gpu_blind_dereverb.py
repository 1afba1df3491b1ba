"""-m gpu: blind dereverberation (csrc/fir_blind.hip, the response stride of csrc/fir.hip, BlindDereverberationOperator).

Kernel level: the weight gradient against float64 autograd, the adjoint identities in h and in x, the per-clip FIR against the shared one,
determinism (twice, batch position, both bindings) and the Adam + peak-normalisation update against the float64 lines of the issue.
Operator level: a frozen estimate equals MusicDereverberationOperator pinned to it bit for bit, one live step moves the estimate by the
float64 first Adam step, and 200 steps on a known clip recover the response.  Step / call level: DPS and DSG steps equal the pinned
operator's, and the pipeline runs it deterministically, under both bindings and in track mode.

The oracle is local: float64 torch, conv1d with padding n // 2 and groups = B."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_step import HIFI, VAE, SCHED, H, W as LAT_W, LEN               # noqa: E402

WGRAD_SHAPES = [(1, 2048, 2048, 1), (2, 2048, 2080, 2), (3, 1000, 1024, 127), (3, 4099, 4200, 128), (2, 4099, 4200, 129),
                (2, 4096, 4096, 513), (1, 6400, 6432, 800), (2, 9000, 9000, 1025), (1, 2048, 2048, 5000)]


def _out_len(L, n):
    return L + 2 * (n // 2) - n + 1


def ref_fwd(x, h):
    """float64: y[b, o] = sum_t h[b, t] x[b, o + t - n // 2];  x (B, L), h (B, n)."""
    B, n = h.shape
    return torch.nn.functional.conv1d(x[None], h[:, None, :], padding=n // 2, groups=B)[0]


def ref_wgrad(dy, x, n):
    """float64 autograd of <dy, A_h x> in h."""
    h = torch.zeros(x.shape[0], n, dtype=torch.float64, requires_grad=True)
    (ref_fwd(x, h) * dy).sum().backward()
    return h.grad


def ref_update(g, h, m, v, k, lr=0.05, b1=0.9, b2=0.999, eps=1e-8):
    """The update lines of the issue in float64, per clip; a clip with a non-finite g or h', or a zero peak, is returned unchanged."""
    g, h, m, v = g.double(), h.double(), m.double(), v.double()
    mn = b1 * m + (1 - b1) * g
    vn = b2 * v + (1 - b2) * g * g
    hp = h - lr * (mn / (1 - b1 ** k)) / (torch.sqrt(vn / (1 - b2 ** k)) + eps)
    peak = hp.abs().amax(dim=1, keepdim=True)
    keep = ~(torch.isfinite(g).all(1, keepdim=True) & torch.isfinite(hp).all(1, keepdim=True) & (peak > 0))
    return torch.where(keep, h, hp / peak), torch.where(keep, m, mn), torch.where(keep, v, vn)


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-300))


def _inputs(B, L, full, n, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    x = 0.1 * torch.randn(B, full, generator=g)
    dy = torch.randn(B, _out_len(L, n), generator=g)
    h = torch.randn(B, n, generator=g)
    return x, dy, h / h.abs().amax(dim=1, keepdim=True)


def _hip():
    from diffmusic_amd import ops
    return ops.load()


# ---- 1. weight gradient -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,full,n", WGRAD_SHAPES)
def test_wgrad_matches_float64(B, L, full, n):
    """Relative L2 over dh <= 1e-5: sequential fp32 accumulation is about 2^-24 sqrt(Lout) = 6e-6 at Lout = 9000, a dropped term or an
    off-by-one tap about 1 / sqrt(Lout) >= 1e-2."""
    x, dy, _ = _inputs(B, L, full, n)
    part = _hip().fir_wgrad(dy.cuda(), x.cuda(), L, n)
    Lout = _out_len(L, n)
    assert part.shape == (B, -(-Lout // 4096), n)
    if (L, n) == (9000, 1025):
        assert part.shape[1] == 3 and Lout % 4096 != 0 and n > 1024      # three segments, the last ragged; two tap tiles of 1024
    ref = ref_wgrad(dy.double(), x[:, :L].double(), n)
    err = _rel(part.double().sum(1), ref)
    print(f"wgrad B={B} L={L} n={n}: rel-L2 {err:.2e}")
    assert err <= 1e-5, err


# ---- 2. adjoints --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,full,n", [(2, 4099, 4200, 129), (2, 9000, 9000, 1025), (3, 1000, 1024, 127), (1, 2048, 2048, 5000)])
def test_adjoint_identities(B, L, full, n):
    h_ = _hip()
    x, dy, h = _inputs(B, L, full, n, seed=1)
    xd, dyd, hd = x.cuda(), dy.cuda(), h.cuda()
    y = h_.fir_clip_fwd(xd, hd, L)
    dh = h_.fir_wgrad(dyd, xd, L, n).double().sum(1)
    dx = h_.fir_clip_bwd(dyd, hd, torch.flip(hd, dims=[1]).contiguous(), L, full)
    assert dx.shape == (B, full) and not dx[:, L:].any()
    lhs = float((dy.double() * y.double().cpu()).sum())
    in_h = float((h.double() * dh.cpu()).sum())
    in_x = float((x[:, :L].double() * dx[:, :L].double().cpu()).sum())
    print(f"adjoint n={n}: <dy, A x> {lhs:.9e}  <h, wgrad> {in_h:.9e}  <x, A^T dy> {in_x:.9e}")
    assert abs(lhs - in_h) <= 1e-5 * abs(lhs) and abs(lhs - in_x) <= 1e-5 * abs(lhs)


# ---- 3. per-clip FIR ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,full,n", [(3, 4099, 4200, 129), (2, 1000, 1024, 64), (2, 6400, 6432, 800), (3, 2048, 2048, 128)])
def test_per_clip_fir_is_the_shared_fir_clip_by_clip(B, L, full, n):
    """Dense (n >= 128) and short-filter kernels: a repeated response gives the bits of resample_fwd / resample_bwd (orig = new = 1), and
    with distinct responses every clip has the bits of its own single-clip call."""
    h_ = _hip()
    x, dy, h = _inputs(B, L, full, n, seed=2)
    xd, dyd, hd = x.cuda(), dy.cuda(), h.cuda()
    Lout, off = _out_len(L, n), n // 2
    one = hd[:1].contiguous()
    rep, rev1 = one.repeat(B, 1), torch.flip(one, dims=[1]).contiguous()
    assert torch.equal(h_.fir_clip_fwd(xd, rep, L), h_.resample_fwd(xd, one, L, Lout, 1, 1, off))
    assert torch.equal(h_.fir_clip_bwd(dyd, rep, rev1.repeat(B, 1), L, full), h_.resample_bwd(dyd, one, rev1, L, full, 1, 1, off))
    rev = torch.flip(hd, dims=[1]).contiguous()
    y, dx = h_.fir_clip_fwd(xd, hd, L), h_.fir_clip_bwd(dyd, hd, rev, L, full)
    assert _rel(y, ref_fwd(x[:, :L].double(), h.double())) <= 1e-5
    for b in range(B):
        hb, rb = hd[b:b + 1].contiguous(), rev[b:b + 1].contiguous()
        assert torch.equal(y[b:b + 1], h_.fir_clip_fwd(xd[b:b + 1], hb, L))
        assert torch.equal(y[b:b + 1], h_.resample_fwd(xd[b:b + 1], hb, L, Lout, 1, 1, off))
        assert torch.equal(dx[b:b + 1], h_.fir_clip_bwd(dyd[b:b + 1].contiguous(), hb, rb, L, full))


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------------------
def test_wgrad_is_deterministic_and_independent_of_the_batch():
    from diffmusic_amd import ops
    h_ = _hip()
    B, L, full, n = 3, 9000, 9040, 1025
    x, dy, h = _inputs(B, L, full, n, seed=3)
    xd, dyd = x.cuda(), dy.cuda()
    a, b = h_.fir_wgrad(dyd, xd, L, n), h_.fir_wgrad(dyd, xd, L, n)
    assert torch.equal(a, b)
    alone = h_.fir_wgrad(dyd[2:3].contiguous(), xd[2:3].clone(), L, n)               # position 0 of 1, another row stride base
    assert torch.equal(alone[0], a[2])
    first = h_.fir_wgrad(torch.cat([dyd[2:3], dyd[:2]]).contiguous(), torch.cat([xd[2:3], xd[:2]]).contiguous(), L, n)
    assert torch.equal(first[0], a[2]) and torch.equal(first[1], a[0])
    c = ops.ctypes_hip.fir_wgrad(dyd, xd, L, n)
    assert torch.equal(a, c)
    hd = h.cuda()
    rev = torch.flip(hd, dims=[1]).contiguous()
    assert torch.equal(h_.fir_clip_fwd(xd, hd, L), ops.ctypes_hip.fir_clip_fwd(xd, hd, L))
    assert torch.equal(h_.fir_clip_bwd(dyd, hd, rev, L, full), ops.ctypes_hip.fir_clip_bwd(dyd, hd, rev, L, full))
    state = [hd.clone(), rev.clone(), 0.1 * torch.randn_like(hd), (0.1 * torch.randn_like(hd)) ** 2]
    s1, s2 = [t.clone() for t in state], [t.clone() for t in state]
    h_.ir_update(a, *s1, 3, 0.05, 0.9, 0.999, 1e-8)
    ops.ctypes_hip.ir_update(a, *s2, 3, 0.05, 0.9, 0.999, 1e-8)
    assert all(torch.equal(p, q) for p, q in zip(s1, s2)) and not torch.equal(s1[0], state[0])


# ---- 5. update ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 7])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 800, 5000])
def test_ir_update_matches_float64(n, k):
    """h within 1e-6 absolute (values <= 1 after the projection, about ten fp32 roundings of 6e-8), m and v within 1e-6 relative (L2 per
    clip: m's two terms can cancel in single elements), h_rev the exact flip, and a clip with a NaN partial untouched."""
    h_ = _hip()
    B, S = 3, 3
    g = torch.Generator().manual_seed(50 + n + k)
    h = torch.randn(B, n, generator=g)
    h = (h / h.abs().amax(dim=1, keepdim=True)).cuda()
    m = (0.1 * torch.randn(B, n, generator=g)).cuda()
    v = ((0.1 * torch.randn(B, n, generator=g)) ** 2).cuda()
    part = (0.05 * torch.randn(B, S, n, generator=g)).cuda()
    part[1, 1, 5 % n] = float("nan")
    rev = torch.flip(h, dims=[1]).contiguous()
    h0, r0, m0, v0 = h.clone(), rev.clone(), m.clone(), v.clone()
    rh, rm, rv = ref_update(part.double().sum(1), h0, m0, v0, k)
    h_.ir_update(part, h, rev, m, v, k, 0.05, 0.9, 0.999, 1e-8)
    assert torch.equal(h[1], h0[1]) and torch.equal(rev[1], r0[1]) and torch.equal(m[1], m0[1]) and torch.equal(v[1], v0[1])
    assert torch.equal(rev, torch.flip(h, dims=[1]))
    for b in (0, 2):
        dh = float((h[b].double() - rh[b]).abs().max())
        em, ev = _rel(m[b], rm[b]), _rel(v[b], rv[b])
        print(f"ir_update n={n} k={k} clip {b}: max|dh| {dh:.2e}  m {em:.2e}  v {ev:.2e}")
        assert not torch.equal(h[b], h0[b]) or n == 1
        assert dh <= 1e-6 and em <= 1e-6 and ev <= 1e-6
        assert float(h[b].abs().max()) == 1.0


def test_ir_update_refuses_more_taps_than_one_workgroup_holds():
    h_ = _hip()
    z = torch.zeros(1, 8193, device="cuda")
    with pytest.raises(RuntimeError, match="8192"):
        h_.ir_update(torch.zeros(1, 1, 8193, device="cuda"), z.clone(), z.clone(), z.clone(), z.clone(), 1, 0.05, 0.9, 0.999, 1e-8)


# ---- 6 / 7. operator ----------------------------------------------------------------------------------------------------------------------
N_OP = 800


def _clip_pair(seed=77):
    g = torch.Generator().manual_seed(seed)
    clean = 0.3 * torch.sin(torch.arange(LEN) * 0.05)[None] * torch.tensor([[1.0], [0.6]]) + 0.05 * torch.randn(2, LEN, generator=g)
    wav = torch.nn.functional.pad(clean + 0.02 * torch.randn(2, LEN, generator=g), (0, 32))    # a vocoder output: LEN + 32 samples
    est = torch.cumsum(torch.randn(N_OP, generator=g), 0) * 0.85
    true = torch.cumsum(torch.randn(N_OP, generator=g), 0) * 0.85
    return clean, wav, est / est.abs().max(), true / true.abs().max()


@pytest.mark.parametrize("space", ["wav_form", "mel_spectrogram"])
def test_frozen_estimate_equals_the_pinned_operator(space):
    from diffmusic_amd import inverse_problem as P
    clean, wav, est, true = _clip_pair()
    blind = P.BlindDereverberationOperator(N_OP, init=est)
    known = P.MusicDereverberationOperator(N_OP)
    y = blind.forward(clean.cuda(), ir=true)
    assert torch.equal(y, known.forward(clean.cuda(), ir=true)) and torch.equal(blind.true_ir, true[None].expand(2, -1))
    wd = wav.cuda()
    loss, dwav = blind.guidance(wd, LEN, y, space, update_ir=False)
    rloss, rdwav = known.guidance(wd, LEN, y, space, ir=est)
    assert torch.equal(loss, rloss) and torch.equal(dwav, rdwav) and dwav.shape == wd.shape and bool(dwav.abs().max() > 0)
    assert blind.k == 0 and torch.equal(blind.ir_estimate.cpu(), est[None].expand(2, -1)) and not blind._m.any()
    loss2, dwav2 = blind.guidance(wd, LEN, y, space, ir=est)                          # a pinned response never updates either
    assert torch.equal(loss2, rloss) and torch.equal(dwav2, rdwav) and blind.k == 0


def test_one_live_step_in_wav_form():
    """Loss and gradient are those of h_0; afterwards the estimate is the float64 first Adam step from h_0.  Bound per tap: item 5's 1e-6
    plus item 1's 1e-5 ||g|| carried through d/dg [g / (|g| + eps)] = eps / (|g| + eps)^2, which is nothing unless |g| is about eps."""
    from diffmusic_amd import inverse_problem as P
    clean, wav, est, true = _clip_pair()
    lr, eps = 0.05, 1e-8
    blind, frozen = P.BlindDereverberationOperator(N_OP, init=est, lr=lr), P.BlindDereverberationOperator(N_OP, init=est, lr=lr)
    y = blind.forward(clean.cuda(), ir=true)
    wd = wav.cuda()
    rloss, rdwav = frozen.guidance(wd, LEN, y, "wav_form", update_ir=False)
    h0 = frozen.ir_estimate.clone()
    loss, dwav = blind.guidance(wd, LEN, y, "wav_form")
    assert torch.equal(loss, rloss) and torch.equal(dwav, rdwav)
    assert blind.k == 1 and not torch.equal(blind.ir_estimate, h0)
    x64, h64 = wav[:, :LEN].double(), h0.double().cpu()
    res = y.double().cpu() - ref_fwd(x64, h64)
    dy = -res / res.norm(dim=1, keepdim=True)
    g = ref_wgrad(dy, x64, N_OP)
    rh, _, _ = ref_update(g, h64, torch.zeros_like(h64), torch.zeros_like(h64), 1, lr=lr, eps=eps)
    peak = (h64 - lr * g / (g.abs() + eps)).abs().amax(dim=1, keepdim=True)
    tol = 1e-6 + lr * eps / (g.abs() + eps) ** 2 * 1e-5 * g.norm(dim=1, keepdim=True) / peak
    diff = (blind.ir_estimate.double().cpu() - rh).abs()
    print(f"live step: max|dh| {float(diff.max()):.2e}, max of diff / tol {float((diff / tol).max()):.3f}, min|g| {float(g.abs().min()):.2e}")
    assert bool((diff <= tol).all())
    assert torch.equal(blind._h_rev, torch.flip(blind.ir_estimate, dims=[1]))
    blind.reset_cache()
    assert torch.equal(blind.ir_estimate, h0) and torch.equal(blind._h_rev, torch.flip(h0, dims=[1])) and blind.k == 0
    assert not blind._m.any() and not blind._v.any()


# ---- 8. recovery --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L", [(64, 4096), (65, 4099)])
def test_estimate_recovers_a_known_response(n, L):
    """No networks: x known and fixed, 200 wav_form steps from the impulse.  The float64 / fp32 CPU restatements of this loop with these seeds end at
    0.004 .. 0.007 (both sizes, both precisions) from 0.98 .. 1.10; the iterates diverge between precisions, the error does not."""
    from diffmusic_amd import inverse_problem as P
    torch.manual_seed(n)
    op = P.BlindDereverberationOperator(n, 0.85, lr=0.05)
    true = torch.cat([op.generate_impulse_response(n, 0.85) for _ in range(2)])
    x = (0.1 * torch.randn(2, L, generator=torch.Generator().manual_seed(5))).cuda()
    y = op.forward(x, ir=true)

    def err():
        return torch.linalg.vector_norm(op.ir_estimate.cpu() - true, dim=1) / torch.linalg.vector_norm(true, dim=1)
    op.reset_cache()
    op.apply(x, L)                                             # fixes the batch: the impulse start exists
    start = err()
    for _ in range(200):
        op.guidance(x, L, y, "wav_form")
    end = err()
    print(f"recovery n={n} L={L}: relative error {start.tolist()} -> {end.tolist()}")
    assert op.k == 200 and bool((start >= 0.9).all()) and bool((end <= 0.05).all())


# ---- 9. scheduler step --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets():
    from diffmusic_amd.engine import HifiGanEngine, VaeDecoderEngine
    voc, vae = HifiGanEngine(HIFI), VaeDecoderEngine(VAE)
    voc.load_state_dict(voc.synth_state_dict(seed=1))
    vae.load_state_dict(vae.synth_state_dict(seed=2))
    return voc, vae


@pytest.mark.parametrize("per_clip", [True, False])
@pytest.mark.parametrize("name,eta,rate", [("dps", 0.0, 5e-4), ("dsg", 1.0, 0.08)])
def test_scheduler_step_equals_the_pinned_operator(nets, name, eta, rate, per_clip):
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    voc, vae = nets
    clean, _, est, true = _clip_pair()
    blind, known = P.BlindDereverberationOperator(N_OP, init=est), P.MusicDereverberationOperator(N_OP)
    y = blind.forward(clean.cuda(), ir=true)
    g = torch.Generator().manual_seed(9)
    x, e, z = (torch.randn(2, 8, H, LAT_W, generator=g).cuda() for _ in range(3))
    outs = []
    for op, opk in ((blind, None), (known, dict(ir=est))):
        s = get_scheduler(name)(operator=op, per_clip_norm=per_clip, **SCHED)
        s.set_timesteps(200)
        noise_kw = dict(sample_noise=z) if name == "dsg" else {}
        outs.append(s.step(e, 501, x, measurement=y, vae=vae, vocoder=voc, op_kwargs=opk, eta=eta, ip_guidance_rate=rate,
                           original_waveform_length=LEN, supervised_space="mel_spectrogram", **noise_kw))
    assert torch.equal(outs[0].prev_sample, outs[1].prev_sample) and torch.equal(outs[0].loss, outs[1].loss)
    assert bool(torch.isfinite(outs[0].prev_sample).all()) and not torch.equal(outs[0].prev_sample, x)
    assert blind.k == 1 and not torch.equal(blind.ir_estimate.cpu(), est[None].expand(2, -1))


# ---- 10. pipeline -------------------------------------------------------------------------------------------------------------------------
N_CALL, SECONDS = 4, 0.4


def _pipe(op, per_clip=True):
    from diffmusic_amd.pipelines import get_pipeline
    from diffmusic_amd.schedulers import get_scheduler
    from tests.test_gpu_warm_start import HIFI as HIFI_SR, UNET
    pipe = get_pipeline("musicldm").from_pretrained("synthetic", seed=0, unet_config=UNET, vae_config=VAE, vocoder_config=HIFI_SR).to("cuda")
    pipe.scheduler = get_scheduler("dps")(operator=op, per_clip_norm=per_clip, **SCHED)
    pipe.assume_uncond_equals_cond = True
    return pipe


@pytest.mark.parametrize("torch_ops", [True, False])
def test_pipeline_call_is_finite_moves_the_estimate_and_repeats(monkeypatch, torch_ops):
    from diffmusic_amd import inverse_problem as P, ops
    monkeypatch.setattr(ops, "USE_TORCH_OPS", torch_ops)
    clean, _, _, true = _clip_pair()
    op = P.BlindDereverberationOperator(N_OP, 0.85, noiser=P.get_noiser("gaussian", 0.0))
    pipe = _pipe(op)
    y = op.forward(clean.cuda(), ir=true)
    pe = torch.nn.functional.normalize(torch.randn(2, 512, generator=torch.Generator().manual_seed(4)), dim=-1)

    def call():
        gens = [torch.Generator().manual_seed(300 + k) for k in range(2)]
        out = pipe(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0,
                   generator=gens, output_type="pt").audios
        return out, op.ir_estimate.clone()
    a, est_a = call()
    assert a.shape == (2, LEN) and bool(torch.isfinite(a).all()) and pipe.nan_restarts == 0 and op.k == N_CALL
    start = torch.zeros(2, N_OP)
    start[:, N_OP // 2] = 1.0
    assert bool(torch.isfinite(est_a).all()) and not torch.equal(est_a.cpu(), start) and bool((est_a.abs().amax(dim=1) == 1.0).all())
    b, est_b = call()
    assert torch.equal(a, b) and torch.equal(est_a, est_b)


def test_pipeline_restarts_the_estimate_with_the_trajectory(monkeypatch):
    """NaN-retry: the trajectory starts again from fresh latents, and the estimate from its start (k counts the last attempt only)."""
    from diffmusic_amd import inverse_problem as P
    clean, _, _, true = _clip_pair()
    op = P.BlindDereverberationOperator(N_OP, 0.85)
    pipe = _pipe(op)
    y = op.forward(clean.cuda(), ir=true)
    pe = torch.nn.functional.normalize(torch.randn(2, 512, generator=torch.Generator().manual_seed(4)), dim=-1)
    real, calls, seen = pipe.scheduler.step, [0], []

    def step(*a, **k):
        seen.append(op.k)
        out = real(*a, **k)
        calls[0] += 1
        if calls[0] == 2:
            out.loss = out.loss * float("nan")
        return out
    monkeypatch.setattr(pipe.scheduler, "step", step)
    pipe(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0,
         generator=[torch.Generator().manual_seed(k) for k in range(2)], output_type="pt")
    assert pipe.nan_restarts == 1 and seen == [0, 1, 0, 1, 2, 3] and op.k == N_CALL


def test_track_mode_call_with_a_batch_one_estimate():
    from diffmusic_amd import inverse_problem as P
    T, R = 11200, 1600                                        # two windows of LEN = 6400 at 0 and 4800
    lay = P.TrackLayout(T, LEN, R)
    assert lay.num_windows == 2
    inner = P.BlindDereverberationOperator(N_OP, 0.85)
    top = P.TrackOperator(inner, lay)
    pipe = _pipe(top, per_clip=False)
    g = torch.Generator().manual_seed(8)
    clean = 0.3 * torch.sin(torch.arange(T) * 0.05)[None] + 0.05 * torch.randn(1, T, generator=g)
    torch.manual_seed(3)
    y = top.forward(clean.cuda())                             # draws the true response of the one track
    assert inner.true_ir.shape == (1, N_OP) and y.shape == (1, T + 1)
    pe = torch.nn.functional.normalize(torch.randn(2, 512, generator=g), dim=-1)
    out = pipe(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0,
               generator=[torch.Generator().manual_seed(k) for k in range(2)], output_type="pt").audios
    assert out.shape == (1, T) and bool(torch.isfinite(out).all())
    est = inner.ir_estimate
    assert est.shape == (1, N_OP) and inner.k == N_CALL and float(est.abs().max()) == 1.0 and int((est != 0).sum()) > 1
