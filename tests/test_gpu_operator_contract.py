"""-m gpu: the operator contract of diffmusic_amd/inverse_problem/operator.py at small shapes (B = 2).

1. `guidance` is the composition of its parts: `apply` -> `noise_add` -> transform / `l2_loss` / transform_bwd -> `adjoint`, written out
   by hand from the public front-end methods, in both supervised spaces, with and without an injected step noise, at a length the fused
   STFT-mel kernels take (2048 = 2 * n_fft, the smallest) and one they do not (1600).
   Where `guidance` materialises y = A(wav) the hand-written chain makes the same launches on the same inputs and has to agree bit for
   bit.  Where y itself is long enough for the fused pair (`frontend.guidance` on y: super-resolution of 4096, dereverberation of 2048)
   "the same launches" is that pair; these cases are held against the transform_fwd / l2_loss / transform_bwd chain as well, to the
   1e-5 that tests/test_gpu_stft_mel.py asserts between the fused pair and that chain.
   Where A rides inside the fused kernels (identity, inpainting, declipping in mel space at 2048) y never exists: same 1e-5.
2. The transpose is a transpose (<A x, w> = <x, A^T w>, float64 accumulation) and belongs to ITS `apply` call: called after a later
   `apply` on another input (of another length, with another impulse response) it returns the same bits as when called at once.
3. `forward` is `apply` plus the noiser."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, PAD = 2, 32                       # rows of length + PAD samples: the vocoder's output is longer than the clip
SIGMA = 0.05
OPERATORS = ("identity", "inpainting", "declipping", "super_resolution", "dereverberation", "phase_retrieval")
ON_LOAD = ("identity", "inpainting", "declipping")      # A inside the fused mel kernels where the clip is long enough for them


def _wave(seed, n, freq):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float32)
    rows = [0.3 * torch.sin(t * freq * (1.0 + 0.37 * b) + b) * (1.0 + 0.3 * torch.sin(t * 0.0007)) + 0.05 * torch.randn(n, generator=g)
            for b in range(B)]
    return torch.stack(rows).cuda().contiguous()


def _ir(seed, taps=800):
    g = torch.Generator().manual_seed(seed)
    ir = torch.cumsum(torch.randn(taps, generator=g), dim=0) * 0.85
    return (ir / ir.abs().max())[None]


def _lengths(name):
    return (4096, 2048) if name == "super_resolution" else (2048, 1600)    # y = A(wav) on each side of 2048 for the resampler too


def _operator(name, length):
    """-> (operator without a noiser, keywords of `apply`)."""
    from diffmusic_amd import inverse_problem as P
    if name == "identity":
        return P.IdentityOperator(16000), {}
    if name == "inpainting":                                   # box hole over samples 480 .. 960
        return P.MusicInpaintingOperator(P.seconds_for_samples(length, 16000), 16000, "box", 0.03, 0.06, 0.3, 0.1, 0.2), {}
    if name == "declipping":
        return P.DeclippingOperator(16000, torch.tensor([0.15, 0.25])), {}
    if name == "super_resolution":
        return P.SuperResolutionOperator(16000, 2), {}
    if name == "dereverberation":
        return P.MusicDereverberationOperator(ir_length=800), dict(ir=_ir(7))
    return P.PhaseRetrievalOperator(), {}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _chain(op, wav, length, meas, space, z, kw, fused_pair_on_y):
    """The guided step by hand.  fused_pair_on_y: take `frontend.guidance` on the materialised y where it is long enough for the fused
    kernels (the launches `guidance` makes); False: transform_fwd / l2_loss / transform_bwd at every length."""
    from diffmusic_amd import ops
    from diffmusic_amd.inverse_problem.operator import l2_loss
    y, adjoint = op.apply(wav, length, **kw)
    if z is not None:
        y = ops.hip.noise_add(y, z, SIGMA)
    if space == "wav_form":
        loss, dy = l2_loss(meas.reshape(B, -1).contiguous(), y.reshape(B, -1))
        return loss, adjoint(dy.reshape(y.shape), wav.shape[1])
    fe, (lo, hi) = op.frontend, op.clamp
    ref = fe.transform_fwd(meas, meas.shape[1], True, True, lo, hi).clone()
    if fused_pair_on_y and fe.fused(y.shape[1]):
        loss, dy = fe.guidance(y, y.shape[1], ref, None, True, True, lo, hi)
    else:
        loss, dmel = l2_loss(ref, fe.transform_fwd(y, y.shape[1], True, True, lo, hi))
        dy = fe.transform_bwd(dmel)
    return loss, adjoint(dy, wav.shape[1])


@pytest.mark.parametrize("name", OPERATORS)
def test_guidance_is_the_composition_of_its_parts(name):
    from diffmusic_amd import inverse_problem as P
    for length in _lengths(name):
        op, kw = _operator(name, length)
        wav, clean = _wave(1, length + PAD, 0.05), _wave(2, length, 0.083)
        meas = op.forward(clean, **kw)                        # no noiser yet: a noiseless measurement, this test is about the step
        g = torch.Generator().manual_seed(3)
        z = torch.randn(op.apply(wav, length, **kw)[0].shape, generator=g).cuda()
        for space in ("wav_form",) if name == "phase_retrieval" else ("wav_form", "mel_spectrogram"):
            for sigma in (0.0, SIGMA):
                case = (name, length, space, sigma)
                op.noiser = P.GaussianNoise(sigma)
                noise = z if sigma > 0 else None
                loss, dwav = op.guidance(wav, length, meas, space, noise=noise, **kw)
                assert loss.shape == (B,) and dwav.shape == wav.shape and bool(torch.isfinite(dwav).all()), case
                assert float(loss.min()) > 0 and float(dwav[:, length:].abs().max()) == 0.0, case
                on_load = space == "mel_spectrogram" and name in ON_LOAD and op.frontend.fused(length)
                if not on_load:
                    l2, d2 = _chain(op, wav, length, meas, space, noise, kw, fused_pair_on_y=True)
                    assert torch.equal(loss, l2) and torch.equal(dwav, d2), (case, loss, l2, _rel(dwav, d2))
                    if space != "mel_spectrogram" or not op.frontend.fused(z.shape[1]):      # z is shaped like y
                        continue
                l2, d2 = _chain(op, wav, length, meas, space, noise, kw, fused_pair_on_y=False)
                rl, rg = float(((loss - l2).abs() / l2).max()), _rel(dwav, d2)
                print(f"\n  {case}: loss {rl:.2e} grad {rg:.2e}")
                assert rl < 1e-5 and rg < 1e-5, (case, rl, rg)


def _dot(a, b):
    return float((a.double().cpu() * b.double().cpu()).sum())


@pytest.mark.parametrize("name", ["identity", "inpainting", "super_resolution", "dereverberation"])
def test_the_transpose_is_a_transpose_and_is_stateless(name):
    length, other = 2048, (2048 if name in ("identity", "inpainting") else 2400)      # the mask fixes the inpainting length
    op, kw = _operator(name, length)
    x = _wave(4, length + PAD, 0.05)
    y, adjoint = op.apply(x, length, **kw)
    # w = y + noise: <A x, w> is about ||y||^2, far from the cancellation an independent w would leave the comparison to
    w = (y + 0.5 * torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).cuda()).contiguous()
    xt = adjoint(w, length + PAD).clone()
    assert xt.shape == x.shape and float(xt[:, length:].abs().max()) == 0.0
    lhs, rhs = _dot(y, w), _dot(x, xt)
    assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), abs(rhs)), (name, lhs, rhs)
    kw2 = dict(ir=_ir(8, 500)) if name == "dereverberation" else {}
    y2, adjoint2 = op.apply(_wave(6, other + PAD, 0.11), other, **kw2)
    assert torch.equal(adjoint(w, length + PAD), xt), name                            # the first call's transpose, after the second call
    assert adjoint2(y2, other + PAD).shape == (B, other + PAD)


def test_the_declipping_transpose_keeps_the_point_it_was_taken_at():
    length = 2048
    op, _ = _operator("declipping", length)
    x = _wave(4, length + PAD, 0.05)
    y, adjoint = op.apply(x, length)
    thr = op.threshold[:, None].cuda()
    inside = x[:, :length].abs() <= thr
    share = inside.float().mean(dim=1)
    assert bool(((share > 0.05) & (share < 0.95)).all()), share                       # both sides of the threshold, in every clip
    assert torch.equal(y, torch.clamp(x[:, :length], -thr, thr))
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).cuda()
    want = torch.zeros_like(x)
    want[:, :length] = torch.where(inside, w, torch.zeros_like(w))                   # the clip mask of the FIRST input
    assert torch.equal(adjoint(w, length + PAD), want)
    x2 = _wave(6, length + PAD, 0.11)
    assert not torch.equal(x2[:, :length].abs() <= thr, inside)
    op.apply(x2, length)
    assert torch.equal(adjoint(w, length + PAD), want)


@pytest.mark.parametrize("name", OPERATORS[1:])
def test_forward_is_apply_plus_the_noiser(name):
    from diffmusic_amd import inverse_problem as P
    n = 2048
    op, kw = _operator(name, n)
    op.noiser = P.GaussianNoise(0.0)
    x = _wave(9, n, 0.05)
    assert torch.equal(op.forward(x, **kw), op.apply(x, n, **kw)[0])
    if name == "inpainting":
        with pytest.raises(ValueError, match="mask length"):
            op.forward(_wave(9, n + 1, 0.05))
