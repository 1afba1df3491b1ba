"""-m gpu: the vocoder under an inpainting hole (`HifiGanEngine.forward(mel, dead=(s0, s1))`, csrc/hifigan.hip DeadPlan) against the
same engine with the feature switched off, bit for bit.

Every row that is still computed runs the instructions it always ran, so nothing here is a tolerance: the waveform outside the
hole, the input gradient and the per-clip loss are EQUAL with the feature on and off, the waveform inside the hole is exactly zero,
and none of it depends on what the workspace held before the call.

The synthetic vocoder has one generic stage (C = 256) and the three pair-kernel stages (C = 128 / 64 / 32), so both seams between
kernels that skip rows and kernels that compute every row are crossed in both directions.  16 x 400 frames = 6400 samples: 7 / 13 /
26 slabs per clip in the three narrow stages, holes of ~3500 samples skip at least one whole slab in each of them (asserted) and leave
a partly dead slab on either side."""
import pytest
import torch

pytestmark = pytest.mark.gpu

VOC = dict(model_in_dim=64, upsample_initial_channel=512, upsample_rates=[2, 2, 2, 2], upsample_kernel_sizes=[4, 4, 4, 4],
           resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5]] * 3, leaky_relu_slope=0.1)
T, LEN = 400, 6400
PAIR_STAGES = (1, 2, 3)                    # C = 128, 64, 32
# (hole, skips): the middle (odd edges, no multiple of any slab height), touching sample 0, touching the last sample, too short to skip
HOLES = [((1501, 5003), True), ((0, 3301), True), ((3099, 6400), True), ((3000, 3200), False)]


def _adt():
    from diffmusic_amd import _lib as L
    return L.act_dtype()


@pytest.fixture(scope="module")
def voc():
    from diffmusic_amd.engine import HifiGanEngine
    eng = HifiGanEngine(VOC)
    eng.load_state_dict(eng.synth_state_dict(seed=5))
    assert eng.out_len(T) == LEN
    return eng


def _Op(hole):
    """The inpainting operator over a mask of this test's choosing."""
    from diffmusic_amd import inverse_problem as P
    op = P.MusicInpaintingOperator(1, LEN, "box", None, None, 0.3, 0.1, 0.2)
    op.mask = torch.ones(1, LEN)
    op.mask[:, hole[0]:hole[1]] = 0.0
    return op


def _inputs(B):
    g = torch.Generator().manual_seed(100 + B)
    mel = (0.7 * torch.randn(B, T, 64, generator=g)).to(_adt()).cuda()
    meas = (0.3 * torch.randn(B, LEN, generator=g)).cuda()
    return mel, meas


def _run(voc, op, mel, meas, on, fill=None):
    """forward -> masked mel loss and its gradient -> backward; fill: byte the workspace is set to before the call."""
    voc.dead_span_enabled = on
    span = op.dead_span(LEN)
    if fill is not None:
        voc._ws["buf"].fill_(fill)
    wav = voc.forward(mel, dead=span)
    plan = voc.dead_plan()
    loss, dwav = op.guidance(wav, LEN, meas, "mel_spectrogram")
    dmel = voc.backward(dwav)
    torch.cuda.synchronize()
    voc.dead_span_enabled = True
    return wav, loss, dwav, dmel, plan


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hole,skips", HOLES, ids=[f"{h[0]}-{h[1]}" for h, _ in HOLES])
def test_on_equals_off(voc, B, hole, skips):
    op = _Op(hole)
    assert op.dead_span(LEN) == hole
    mel, meas = _inputs(B)
    wav0, loss0, dwav0, dmel0, plan0 = _run(voc, op, mel, meas, on=False)
    assert all(p["skipped"] == 0 and p["total"] == 0 for p in plan0)
    assert float(dwav0[:, hole[0]:hole[1]].abs().max()) == 0.0          # what the operator promises with its span
    assert float(wav0[:, hole[0]:hole[1]].abs().max()) > 0.0 and float(dmel0.float().abs().max()) > 0.0     # not vacuous
    wav1, loss1, dwav1, dmel1, plan1 = _run(voc, op, mel, meas, on=True)
    print("\n  hole", hole, "B", B, "plan", plan1)
    if skips:
        for s in PAIR_STAGES:                                            # a whole slab skipped in EVERY pair stage ...
            assert 0 < plan1[s]["skipped"] < plan1[s]["total"], (s, plan1)
            lo, hi = plan1[s]["span"]
            rows = LEN >> (3 - s)
            # ... with a partly dead slab at each edge that lies inside the clip (no slab height, 206 ... 254 rows, divides both edges)
            assert 0 <= lo < hi <= rows and (hi - lo) >= 254
            assert lo == 0 or any(lo % bm for bm in (254, 250, 246)), (s, lo)
            assert hi == rows or any(hi % bm for bm in (254, 250, 246)), (s, hi)
        assert plan1[0]["skipped"] == 0                                  # the generic stage computes every row
        assert float(wav1[:, hole[0]:hole[1]].abs().max()) == 0.0
    else:
        assert all(p["skipped"] == 0 for p in plan1)                     # nothing to gain: the plain path, hole samples included
        assert torch.equal(wav1, wav0)
    keep = torch.ones(LEN, dtype=torch.bool, device="cuda")
    keep[hole[0]:hole[1]] = False
    assert torch.equal(wav1[:, keep], wav0[:, keep])
    assert torch.equal(loss1, loss0) and loss1.shape == (B,)
    assert torch.equal(dwav1, dwav0)
    assert torch.equal(dmel1, dmel0)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hole", [h for h, s in HOLES if s], ids=[f"{h[0]}-{h[1]}" for h, s in HOLES if s])
def test_stale_workspace_never_reaches_a_live_row(voc, B, hole):
    """Skipped rows are never written, so they hold whatever the workspace held: all-ones bytes (NaN in fp16 and fp32) and 0x7b bytes
    (6.3e4 in fp16, 1.3e36 in fp32) must change nothing."""
    op = _Op(hole)
    mel, meas = _inputs(B)
    want = _run(voc, op, mel, meas, on=True)
    assert sum(p["skipped"] for p in want[4]) > 0
    for fill in (0xFF, 0x7B):
        got = _run(voc, op, mel, meas, on=True, fill=fill)
        for a, b in zip(got[:4], want[:4]):
            assert bool(torch.isfinite(a.float()).all())
            assert torch.equal(a, b), fill


def test_a_plain_forward_after_a_dead_one_is_plain(voc):
    """`__call__` and a forward without `dead=` keep the full path, whatever the call before them did."""
    op = _Op(HOLES[0][0])
    mel, meas = _inputs(1)
    _run(voc, op, mel, meas, on=True)
    wav = voc.forward(mel)
    assert all(p["skipped"] == 0 for p in voc.dead_plan())
    voc.dead_span_enabled = False
    assert torch.equal(wav, voc.forward(mel, dead=HOLES[0][0]))
    voc.dead_span_enabled = True
    assert torch.equal(wav, voc(mel))


def test_both_bindings():
    from diffmusic_amd import ops
    from diffmusic_amd.engine import HifiGanEngine
    eng = HifiGanEngine(VOC)
    eng.load_state_dict(eng.synth_state_dict(seed=5))
    mel, _ = _inputs(1)
    hole = HOLES[0][0]
    eng.forward(mel)                                                     # (sizes the workspace)
    ws = eng._ws["buf"]
    wav = ops.load().hifigan_fwd(eng._h.value, mel, ws, hole[0], hole[1])
    plan = list(ops.load().hifigan_dead_plan(eng._h.value, 4))
    assert torch.equal(ops.ctypes_hip.hifigan_fwd(eng._h.value, mel, ws, hole[0], hole[1]), wav)
    assert ops.ctypes_hip.hifigan_dead_plan(eng._h.value, 4) == plan and sum(plan[0::4]) > 0


@pytest.mark.parametrize("sigma", [0.0, 0.05])
def test_teacher_forced_step_on_equals_off(voc, sigma):
    """One DPS inpainting step (VAE decode -> vocoder -> masked mel loss -> back), measurement noise off and on (teacher-forced draw):
    `prev_sample` and `loss` are equal with the feature on and off."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.engine import VaeDecoderEngine
    from diffmusic_amd.schedulers import get_scheduler
    from tests.test_gpu_step import SCHED, VAE
    vae = VaeDecoderEngine(VAE)
    vae.load_state_dict(vae.synth_state_dict(seed=2))
    B, H, W = 2, T // 4, 16
    op = P.MusicInpaintingOperator(1, LEN, "box", 0.2, 0.8, 0.3, 0.1, 0.2, noiser=P.GaussianNoise(sigma) if sigma > 0 else None)
    assert op.dead_span(LEN) == (1280, 5120)
    g = torch.Generator().manual_seed(31)
    x, e = torch.randn(B, 8, H, W, generator=g).cuda(), torch.randn(B, 8, H, W, generator=g).cuda()
    y = op.mask.cuda() * (0.3 * torch.randn(B, LEN, generator=g)).cuda()
    opk = dict(noise=torch.randn(B, LEN, generator=g).cuda()) if sigma > 0 else None
    out = {}
    for on in (False, True):
        voc.dead_span_enabled = on
        sched = get_scheduler("dps")(operator=op, **SCHED)
        sched.set_timesteps(200)
        o = sched.step(e, 501, x, eta=0.0, ip_guidance_rate=5e-4, measurement=y, vae=vae, vocoder=voc, original_waveform_length=LEN,
                       supervised_space="mel_spectrogram", op_kwargs=opk)
        torch.cuda.synchronize()
        out[on] = (o.prev_sample.clone(), o.loss.clone(), voc.dead_plan())
    voc.dead_span_enabled = True
    assert all(out[True][2][s]["skipped"] > 0 for s in PAIR_STAGES) and all(p["skipped"] == 0 for p in out[False][2])
    assert torch.equal(out[True][0], out[False][0])
    assert torch.equal(out[True][1], out[False][1])
    assert bool(torch.isfinite(out[True][0]).all()) and float(out[True][1].min()) > 0.0
    assert not torch.equal(out[True][0], x)
