"""-m gpu: codec restoration (csrc/mdct_quant.hip, inverse_problem/operator.py CodecOperator).

Kernel level: every case of tests/mdct_cases.py in the three modes (QUANT, PASS, PROJECT) through both bindings (bit-identical): the kernel's
codes under the code rule, then EVERY element of the waveform against the float64 model synthesised from the kernel's own codes, within the
bound derived from the number formats; transparent steps give the identity under the bound; exact ties round half to even; reproducibility
and layout; NaN containment; refusals through the C ABI write nothing; grids, clips and codes of arbitrary bits stay inside their buffers.
Operator level: `apply` / `adjoint`, the contract of tests/test_gpu_operator_contract.py, the dead span, `encode` and `project`.  Step
level: teacher-forced steps against `oracle.schedulers` around `OracleCodec` below -- the torch restatement `CodecSTE` of
tests/test_mdct_bound_host.py, whose backward is the straight-through rule -- with the cases and bounds of
tests/test_gpu_declip.py::test_teacher_forced_declipping_step.  Call level: `pipe(...)` equals a hand-written loop bit for bit, alone, inside
a TrackOperator and inside a MixtureOperator; clip lanes with a shared grid equal the plain loop."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import mdct_cases as M                                                      # noqa: E402
from tests.test_mdct_bound_host import CodecSTE                                        # noqa: E402
from tests.test_gpu_step import HIFI, VAE, SCHED, H, W as LAT_W, LEN                   # noqa: E402

CANARY = 12345.678
ICANARY = 1234567
_REPORT = {}


@pytest.fixture(scope="module")
def fe():
    from diffmusic_amd.inverse_problem.operator import SpectralFrontend
    return SpectralFrontend(16000, 1024, 160, 64, "hann")


def _bindings():
    from diffmusic_amd import ops
    return (("torch_ops", ops.load()), ("ctypes", ops.ctypes_hip))


def _step_t(step):
    return torch.from_numpy(np.ascontiguousarray(np.swapaxes(step, -1, -2))).cuda()


def _dev_case(c):
    i = M.inputs(c)
    store = torch.from_numpy(i.store).cuda()                       # (B, stride): clip b at row b
    return i, store[:, :c.full], _step_t(i.step)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _canary_out(B, full, stride, slack=64):
    buf = torch.full((slack + B * stride + slack,), CANARY, dtype=torch.float32, device="cuda")
    return buf, buf[slack:slack + B * stride].view(B, stride)[:, :full]


def _untouched_outside(buf, B, full, stride, slack=64):
    keep = torch.ones(buf.numel(), dtype=torch.bool, device="cuda")
    for b in range(B):
        keep[slack + b * stride: slack + b * stride + full] = False
    return bool((buf[keep] == CANARY).all())


def _run(binding, h, mode, x, dt, c, codes=None, **kw):
    """-> (out, codes) of one mode through one binding"""
    if mode == M.QUANT:
        return binding.mdct_quant(h, x, dt, c.L, c.full, want_codes=True, **kw)
    if mode == M.PASS:
        return binding.mdct_quant(h, x, dt, c.L, c.full, passthrough=True, **kw)
    return binding.mdct_project(h, x, dt, codes, c.L, c.full, **kw), None


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", M.CASES, ids=lambda c: c.name)
def test_kernel_obeys_the_code_rule_and_lies_within_the_bound_in_every_element(fe, c):
    from diffmusic_amd import ops
    i, x, dt = _dev_case(c)
    ref = M.reference(c)
    h = fe._h.value
    pcodes = torch.from_numpy(ref.other_codes.astype(np.int32)).cuda()
    for mode in M.MODES:
        outs = []
        for name, binding in _bindings():
            out, codes = _run(binding, h, mode, x, dt, c, pcodes)
            assert out.shape == (c.B, c.full) and out.is_contiguous()
            assert bool((_bits(out[:, c.L:]) == 0).all()), "out[:, L:full] is +0.0f"
            if mode == M.QUANT:
                assert codes.shape == (c.B, c.T, M.N) and codes.dtype == torch.int32
            outs.append((out, codes))
        assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])), "the two bindings are bit-identical"
        out, codes = outs[0]
        got_codes = None
        if mode == M.QUANT:
            assert torch.equal(codes, outs[1][1])
            got_codes = codes.cpu().numpy().astype(np.int64)
        y = out[:, :c.L].cpu().numpy()
        ratio, broken, differing = M.check(c, mode, y, got_codes)
        _REPORT[(c.name, mode)] = ratio
        print(f"\n  {c.name}/{mode}: largest |kernel - model| / bound = {ratio:.4f}; codes off the rule {broken}, ambiguous and differing "
              f"{differing} of {int(ref.amb.sum())} ambiguous")
        assert broken == 0, (c.name, mode, broken)
        assert ratio <= 1.0, (c.name, mode, ratio)
        if c.step == "zero":                                       # transparent: the identity, element-wise under the bound
            _, bnd = M.expect(i.x, i.step, c.L, M.PASS)
            assert M.ratio(y, i.x.astype(np.float64), bnd) <= 1.0, (c.name, mode)
            if mode == M.QUANT:
                assert (got_codes == M.MARK).all()
        if c.step == "dead_frames" and mode != M.PROJECT:
            assert bool((_bits(out[:, 3072:6144]) == 0).all()), "dead samples are exactly +0.0f"
        # caller-owned strided output: nothing past `full`, or past a row's stride, is written
        buf, view = _canary_out(c.B, c.full, c.out_stride)
        got, _ = _run(ops.ctypes_hip, h, mode, x, dt, c, pcodes, out=view)
        assert got.data_ptr() == view.data_ptr() and torch.equal(_bits(view), _bits(out))
        assert _untouched_outside(buf, c.B, c.full, c.out_stride)


def test_exact_ties_round_half_to_even(fe):
    """With a step 2^(e - 22), e the exponent of the coefficient, C / D is exact and equals M / 2 for the 24-bit significand M of the
    kernel's own C: every odd M is an exact tie, and round-half-even sends all of them to even codes.  So an ODD code proves M = 2 q: there
    C = q D is known exactly, without any second oracle.  A second launch plants steps with fp32 C / D == 2.5 and == 3.5 exactly on such
    coefficients: the codes must be 2 and 4 (times the sign).  A kernel that rounded ties another way would either hand back odd codes whose
    C is not q D (the planted quotients are then no ties and land on both sides) or miss the planted ties themselves.  The share of even
    codes of the first launch is printed only: the low bits of M are not uniform (C ends in a subtraction), so no figure follows for it."""
    from diffmusic_amd import ops
    c = M.CASE["L6400_rand"]
    i, x, _ = _dev_case(c)
    r = M.reference(c).r
    h = fe._h.value
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(r.C)))                         # the model's exponent: the kernel's, unless C sits next to a power of two
    D1 = np.exp2(e - 22).astype(np.float32)                        # (B, T, 512), the kernel's layout
    _, codes = ops.hip.mdct_quant(h, x, torch.from_numpy(D1).cuda(), c.L, c.full, want_codes=True)
    q = codes.cpu().numpy().astype(np.int64)
    ok = (np.abs(q) >= 2 ** 22) & (np.abs(q) < 2 ** 23) & (np.abs(r.C) > 1e-4)      # |q| in [2^22, 2^23): the exponent guess held, C / D = M / 2
    assert ok.mean() > 0.9
    even = float((q[ok] % 2 == 0).mean())
    print(f"\n  even codes under exact halves: {even:.4f} of {int(ok.sum())}")
    known = ok & (q % 2 != 0)
    Ck = (q * D1.astype(np.float64)).astype(np.float32)            # exact: q < 2^23 times a power of two
    assert (Ck.astype(np.float64) == q * D1.astype(np.float64)).all()
    for half, want in ((2.5, 2), (3.5, 4)):
        D2 = np.ones(Ck.shape, np.float32)
        ties = M.plant_tie(np.where(known, Ck, 0.0), half, tries=256)
        assert len(ties) >= 32, len(ties)
        for idx, d in ties:
            D2.reshape(-1)[idx] = d
        _, codes2 = ops.hip.mdct_quant(h, x, torch.from_numpy(D2).cuda(), c.L, c.full, want_codes=True)
        q2 = codes2.cpu().numpy().reshape(-1)
        for idx, _ in ties:
            assert int(q2[idx]) == int(np.sign(Ck.reshape(-1)[idx])) * want, (half, idx, int(q2[idx]))


def test_reproducibility_and_layout(fe):
    from diffmusic_amd import ops
    h = fe._h.value
    for name in ("L4999_rand_pc", "L6400_stride", "L4097_rand", "L6400_lowpass_pc"):
        c = M.CASE[name]
        i, x, dt = _dev_case(c)
        pcodes = torch.from_numpy(M.reference(c).other_codes.astype(np.int32)).cuda()
        for mode in M.MODES:
            first, codes = _run(ops.hip, h, mode, x, dt, c, pcodes)
            again, codes2 = _run(ops.hip, h, mode, x, dt, c, pcodes)
            assert torch.equal(_bits(first), _bits(again)), "two runs are bit-equal"
            for b in range(c.B):                                   # a clip alone = the clip at position b of the batch
                d_b = dt[b] if c.per_clip else dt
                alone, codes_b = _run(ops.hip, h, mode, x[b:b + 1], d_b, c, pcodes[b:b + 1].contiguous())
                assert torch.equal(_bits(alone[0]), _bits(first[b])), (name, mode, b)
                if mode == M.QUANT:
                    assert torch.equal(codes_b[0], codes[b]) and torch.equal(codes, codes2)
            swapped, _ = _run(ops.hip, h, mode, x.flip(0).contiguous(), dt.flip(0).contiguous() if c.per_clip else dt, c, pcodes.flip(0).contiguous())
            assert torch.equal(_bits(swapped.flip(0)), _bits(first)), "batch position does not matter"
            if not c.per_clip:                                     # a shared grid = the same grid repeated per clip
                rep = dt[None].expand(c.B, -1, -1).contiguous()
                assert torch.equal(_bits(_run(ops.hip, h, mode, x, rep, c, pcodes)[0]), _bits(first)), name
    c = M.CASE["L6400_stride"]
    assert c.full > c.L and c.stride > c.full


def test_a_nan_sample_reaches_exactly_its_two_frames(fe):
    from diffmusic_amd import ops
    c = M.CASE["L6400_rand"]
    i, x, dt = _dev_case(c)
    h = fe._h.value
    pcodes = torch.from_numpy(M.reference(c).other_codes.astype(np.int32)).cuda()
    s = 2700                                                       # hop 5: frames 5 and 6, which cover the hops 4 .. 6 = [2048, 3584)
    bad = x.clone()
    bad[1, s] = float("nan")
    for mode in M.MODES:
        clean, ccodes = _run(ops.hip, h, mode, x, dt, c, pcodes)
        out, codes = _run(ops.hip, h, mode, bad, dt, c, pcodes)
        nan = torch.isnan(out[1])
        assert bool(nan[2048:3584].all()) and int(nan.sum()) == 1536, (mode, int(nan.sum()))
        keep = torch.ones(c.L, dtype=torch.bool, device="cuda")
        keep[2048:3584] = False
        assert torch.equal(_bits(out[1, :c.L][keep]), _bits(clean[1, :c.L][keep])) and torch.equal(_bits(out[0]), _bits(clean[0])), mode
        if mode == M.QUANT:                                        # the NaN coefficients pass through with the mark, the others keep their codes
            assert bool((codes[1, 5:7] == M.MARK).all())
            same = torch.ones(c.T, dtype=torch.bool, device="cuda")
            same[5:7] = False
            assert torch.equal(codes[1, same], ccodes[1, same]) and torch.equal(codes[0], ccodes[0])


def _raw(lib, B, L, full, T):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(handle, x, d, mode=M.QUANT, xs=None, ds=0, os_=None, L_=L, full_=full, batch=B, null=(), codes_in=None):
        """-> (rc, out untouched, codes untouched, out view, codes view)"""
        os_ = full if os_ is None else os_
        buf, view = _canary_out(B, full, full)
        cbuf = torch.full((64 + B * T * 512 + 64,), ICANARY, dtype=torch.int32, device="cuda")
        if codes_in is not None:
            cbuf[64:64 + B * T * 512] = codes_in.reshape(-1)
        before = cbuf.clone()
        ptr = dict(x=x.data_ptr(), step=d.data_ptr(), out=view.data_ptr(), codes=cbuf[64:].data_ptr())
        for n in null:
            ptr[n] = 0
        xs = x.stride(0) if xs is None else xs
        if mode == M.PROJECT:
            rc = lib.dmx_mdct_project(handle, C.c_void_p(ptr["x"]), xs, C.c_void_p(ptr["step"]), ds, C.c_void_p(ptr["codes"]), C.c_void_p(ptr["out"]),
                                      os_, batch, L_, full_, st)
        else:
            rc = lib.dmx_mdct_quant(handle, C.c_void_p(ptr["x"]), xs, C.c_void_p(ptr["step"]), ds, C.c_void_p(ptr["codes"]), C.c_void_p(ptr["out"]),
                                    os_, batch, L_, full_, 1 if mode == M.PASS else 0, st)
        torch.cuda.synchronize()
        guards_ok = bool((cbuf[:64] == ICANARY).all()) and bool((cbuf[64 + B * T * 512:] == ICANARY).all()) and \
            _untouched_outside(buf, B, full, full)
        return rc, bool((buf == CANARY).all()), torch.equal(cbuf, before), guards_ok, view, cbuf[64:64 + B * T * 512].view(B, T, 512)
    return call


def test_refusals_through_the_c_abi_write_nothing(fe):
    from diffmusic_amd import _lib, ops
    from diffmusic_amd.inverse_problem.operator import SpectralFrontend
    lib = _lib.lib()
    L, full, B = 1500, 1510, 2
    T = lib.dmx_mdct_frames(L)
    assert T == M.frames(L) == 4 and lib.dmx_mdct_frames(0) == 0 and lib.dmx_mdct_frames(160000) == 314
    x = torch.randn(B, full, device="cuda")
    d = torch.full((B, T, 512), 0.1, device="cuda")
    short = SpectralFrontend(16000, 512, 160, 64, "hann")
    call = _raw(lib, B, L, full, T)
    ok = fe._h
    for mode in M.MODES:                                           # the same calls with nothing wrong run
        rc, out_same, codes_same, guards, _, _ = call(ok, x, d, mode)
        assert rc == 0 and not out_same and guards and codes_same == (mode != M.QUANT), mode
    assert call(ok, x, d, ds=T * 512)[0] == 0
    for mode in M.MODES:
        for what, kw in (("n_fft 512", dict(handle=short._h)), ("full < L", dict(full_=L - 1)), ("short x stride", dict(xs=L - 1)),
                         ("short out stride", dict(os_=full - 1)), ("L < 1", dict(L_=0)), ("short step stride", dict(ds=T * 512 - 1)),
                         ("negative step stride", dict(ds=-1)), ("null x", dict(null=("x",))), ("null step", dict(null=("step",))),
                         ("null out", dict(null=("out",))), ("null handle", dict(handle=C.c_void_p(0))), ("batch 0", dict(batch=0)),
                         ("batch 65536", dict(batch=65536))) + ((("null codes", dict(null=("codes",))),) if mode == M.PROJECT else ()):
            kw = dict(kw)
            rc, out_same, codes_same, guards, _, _ = call(kw.pop("handle", ok), x, d, mode, **kw)
            assert rc != 0 and out_same and codes_same and guards, (mode, what)
            assert lib.dmx_last_error(), (mode, what)
    assert call(ok, x, d, M.QUANT, null=("codes",))[0] == 0          # the quantiser's codes are optional
    codes = torch.zeros(B, T, 512, dtype=torch.int32, device="cuda")
    for _, binding in _bindings():                                 # and the bindings' own checks
        for bad in (lambda: binding.mdct_quant(ok.value, x, d[:, :-1].contiguous(), L, full), lambda: binding.mdct_quant(ok.value, x, d, L, L - 1),
                    lambda: binding.mdct_quant(short._h.value, x, d, L, full), lambda: binding.mdct_quant(ok.value, x.cpu(), d, L, full),
                    lambda: binding.mdct_quant(ok.value, x, d[:1].contiguous(), L, full), lambda: binding.mdct_quant(ok.value, x, d.double(), L, full),
                    lambda: binding.mdct_quant(ok.value, x, d, L, full, passthrough=True, want_codes=True),
                    lambda: binding.mdct_project(ok.value, x, d, codes[:, :-1].contiguous(), L, full),
                    lambda: binding.mdct_project(ok.value, x, d, codes.float(), L, full), lambda: binding.mdct_project(ok.value, x, d, codes, full + 1, full + 1)):
            with pytest.raises((RuntimeError, AssertionError)):
                bad()
    assert ops.hip.mdct_quant(ok.value, x, d[0].contiguous(), L, full)[0].shape == (B, full)


def test_arbitrary_bits_stay_inside_their_buffers(fe):
    """The C entries cannot see the values, so the kernel is safe for any bits (read through in csrc/mdct_quant.hip: x, step and codes only
    enter arithmetic and comparisons; every address comes from the frame, the lane and the strides).  NaN, negative, +-inf, denormal and
    huge steps, NaN / inf / denormal samples, arbitrary code words, with guard bands around the output and the codes: the calls return, the
    guards are intact, a negative or NaN step passes the coefficient through with the mark, and the clean clip in the same batch keeps its
    bits.  Nothing here is out of the launch contract."""
    from diffmusic_amd import _lib
    lib = _lib.lib()
    L, full, B = 1500, 1510, 4
    T = M.frames(L)
    rng = np.random.default_rng(9)
    xh = (0.3 * rng.standard_normal((B, full))).astype(np.float32)
    xh[1, 100], xh[1, 900], xh[1, 901] = np.nan, np.inf, 1e-42
    xh[3] = rng.integers(-2 ** 31, 2 ** 31, full, dtype=np.int64).astype(np.int32).view(np.float32)      # any bits
    dh = rng.uniform(0.02, 0.3, (B, T, 512)).astype(np.float32)
    dh[0, :, 0::5], dh[0, :, 1::5], dh[0, :, 2::5], dh[0, :, 3::5] = np.nan, -0.1, -np.inf, 1e-42
    dh[0, :, 4::5] = 3e38
    dh[1, 1] = np.inf
    dh[3] = rng.integers(-2 ** 31, 2 ** 31, (T, 512), dtype=np.int64).astype(np.int32).view(np.float32)
    x, d = torch.from_numpy(xh).cuda(), torch.from_numpy(dh).cuda()
    anycodes = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (B, T, 512), dtype=np.int64).astype(np.int32)).cuda()
    call = _raw(lib, B, L, full, T)
    alone = _raw(lib, 1, L, full, T)
    for mode in M.MODES:
        rc, out_same, _, guards, out, codes = call(fe._h, x, d, mode, ds=T * 512, codes_in=anycodes if mode == M.PROJECT else None)
        assert rc == 0 and not out_same and guards, mode
        assert bool((_bits(out[:, L:]) == 0).all())
        rc1, _, _, g1, out1, codes1 = alone(fe._h, x[2:3].contiguous(), d[2:3].contiguous(), mode, ds=T * 512, batch=1,
                                            codes_in=anycodes[2:3] if mode == M.PROJECT else None)
        assert rc1 == 0 and g1 and torch.equal(_bits(out[2]), _bits(out1[0])) and bool(torch.isfinite(out[2]).all()), mode
        if mode == M.QUANT:
            assert torch.equal(codes[2], codes1[0])
            k = torch.arange(512, device="cuda")
            assert bool((codes[0][:, (k % 5 == 0) | (k % 5 == 1) | (k % 5 == 2)] == M.MARK).all())      # NaN, negative, -inf steps: not coded
            assert bool((codes[1, 1] == 0).all())                                                       # +inf: discarded, code 0
            assert bool(torch.isfinite(out[0]).all())                                                   # clip 0 is finite under any step


def test_report_largest_ratios():
    if _REPORT:
        for mode in M.MODES:
            sub = {k: v for k, v in _REPORT.items() if k[1] == mode}
            worst = max(sub, key=sub.get)
            print(f"\n  {mode}: largest |kernel - model| / bound over {len(sub)} cases: {sub[worst]:.4f} ({worst[0]})")


# ---- operator level -------------------------------------------------------------------------------------------------------------------
def _codec_op(length, per_clip=False, lowpass=True, noiser=None):
    from diffmusic_amd import inverse_problem as P
    grids = []
    for b in range(2 if per_clip else 1):
        g = M.step_test_grid(M.frames(length), lowpass) * np.float32(0.2 * (1 + b))        # steps 0.1 .. 0.2 (0.2 .. 0.4)
        grids.append(g)
    return P.CodecOperator(16000, np.stack(grids) if per_clip else grids[0], noiser=noiser)


def test_apply_and_adjoint(fe):
    from diffmusic_amd import ops
    from tests.test_gpu_operator_contract import B, PAD, _wave, _dot
    length = 2048
    x = _wave(4, length + PAD, 0.05)
    w = _wave(5, length, 0.021)
    # no infinite step: the straight-through transpose is the zero-padded copy, bit for bit
    op = _codec_op(length, lowpass=False)
    assert op.lossless
    y, adjoint = op.apply(x, length)
    assert y.shape == (B, length) and torch.equal(y, ops.hip.mdct_quant(op.frontend._h.value, x, op.step_on(x.device), length, length)[0])
    xt = adjoint(w, length + PAD)
    assert xt.shape == x.shape and torch.equal(_bits(xt[:, :length]), _bits(w)) and bool((_bits(xt[:, length:]) == 0).all())
    assert float((y - x[:, :length]).abs().max()) > 1e-3                              # the quantiser acts
    # a low-pass grid: Phi^T K Phi, symmetric, independent of x
    op = _codec_op(length, per_clip=True)
    assert not op.lossless
    y, adjoint = op.apply(x, length)
    xt = adjoint(w, length + PAD).clone()
    assert torch.equal(xt, ops.hip.mdct_quant(op.frontend._h.value, w, op.step_on(x.device), length, length + PAD, passthrough=True)[0])
    assert float(xt[:, length:].abs().max()) == 0.0 and float((xt[:, :length] - w).abs().max()) > 1e-3
    _, adjoint2 = op.apply(_wave(6, length + PAD, 0.11), length)
    assert torch.equal(adjoint2(w, length + PAD), xt) and torch.equal(adjoint(w, length + PAD), xt)
    v = _wave(7, length, 0.033)
    lhs, rhs = _dot(adjoint(v, length), w), _dot(v, xt[:, :length])
    assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    codes = op.encode(x[:, :length])
    assert codes.shape == (B, M.frames(length), 512) and codes.dtype == torch.int32 and bool((codes[:, :, 256:] == 0).all())
    assert torch.equal(codes, ops.hip.mdct_quant(op.frontend._h.value, x, op.step_on(x.device), length, length, want_codes=True)[1])


@pytest.mark.parametrize("per_clip", [False, True], ids=["shared", "per_clip"])
def test_guidance_is_the_composition_of_its_parts(per_clip, monkeypatch):
    """tests/test_gpu_operator_contract.py for the new operator: `guidance` = apply -> noise_add -> fused pair (2048) or dense chain (1600)
    -> adjoint, bit for bit, both spaces, with and without an injected noise at sigma = 0.05, in both bindings."""
    from diffmusic_amd import inverse_problem as P, ops
    from tests.test_gpu_operator_contract import B, PAD, SIGMA, _wave, _chain
    for length in (2048, 1600):
        for lowpass in (True, False):
            op = _codec_op(length, per_clip, lowpass)
            assert op._on_load(None, length) is None
            wav, clean = _wave(1, length + PAD, 0.05), _wave(2, length, 0.083)
            meas = op.forward(clean)
            assert meas.shape == (B, length)
            z = torch.randn(B, length, generator=torch.Generator().manual_seed(3)).cuda()
            for space in ("wav_form", "mel_spectrogram"):
                for sigma in (0.0, SIGMA):
                    case = (per_clip, length, lowpass, space, sigma)
                    op.noiser = P.GaussianNoise(sigma)
                    noise = z if sigma > 0 else None
                    loss, dwav = op.guidance(wav, length, meas, space, noise=noise)
                    assert loss.shape == (B,) and dwav.shape == wav.shape and bool(torch.isfinite(dwav).all()), case
                    assert float(loss.min()) > 0 and float(dwav[:, length:].abs().max()) == 0.0 and float(dwav.abs().max()) > 0, case
                    l2, d2 = _chain(op, wav, length, meas, space, noise, {}, fused_pair_on_y=True)
                    assert torch.equal(loss, l2) and torch.equal(dwav, d2), case
                    monkeypatch.setattr(ops, "USE_TORCH_OPS", False)   # the other binding: the same bits
                    assert not ops.enabled()
                    l3, d3 = op.guidance(wav, length, meas, space, noise=noise)
                    monkeypatch.setattr(ops, "USE_TORCH_OPS", True)
                    assert torch.equal(loss, l3) and torch.equal(dwav, d3), case
            op.noiser = P.GaussianNoise(0.0)
            assert torch.equal(op.forward(clean), op.apply(clean, length)[0])          # forward is apply plus the noiser
        with pytest.raises(ValueError, match="512"):
            op.forward(_wave(9, length + 512, 0.05))
        with pytest.raises(ValueError, match="512"):
            op.guidance(_wave(9, length + 600, 0.05), length + 512, meas, "wav_form")


@pytest.mark.parametrize("space", ["mel_spectrogram", "wav_form"])
def test_gradient_is_exactly_zero_on_the_dead_span(space):
    from diffmusic_amd import inverse_problem as P
    from tests.test_gpu_operator_contract import _wave
    g = M.step_test_grid(M.frames(LEN), True) * np.float32(0.2)
    g[:, 4:9] = np.inf                                             # frames 4 .. 8: the hops 4 .. 7
    op = P.CodecOperator(16000, g)
    span = op.dead_span(LEN)
    assert span == (2048, 4096)
    wav, clean = _wave(1, LEN + 32, 0.05), _wave(2, LEN, 0.083)
    meas = op.forward(clean)
    assert bool((_bits(meas[:, span[0]:span[1]]) == 0).all())
    loss, dwav = op.guidance(wav, LEN, meas, space)
    assert float(dwav[:, span[0]:span[1]].abs().max()) == 0.0 and float(dwav[:, :span[0]].abs().max()) > 0
    wav2 = wav.clone()
    wav2[:, span[0]:span[1]] = 7.0                                 # A does not see those samples
    loss2, dwav2 = op.guidance(wav2, LEN, meas, space)
    assert torch.equal(loss, loss2) and torch.equal(dwav, dwav2)


def test_project_moves_whole_frames_into_the_cells_and_nothing_else():
    from diffmusic_amd import inverse_problem as P
    c = M.CASE["L6400_coarse_lowpass"]
    i = M.inputs(c)
    op = P.CodecOperator(16000, i.step)
    clean, other = torch.from_numpy(i.x.copy()).cuda(), torch.from_numpy(i.other).cuda()
    y = op.forward(clean)
    codes = op.encode(y).cpu().numpy().astype(np.int64)
    ref = M.reference(c)
    whole = M.whole_frames(c.L, c.T)
    assert not ref.amb.any() and (codes[:, whole] == ref.codes[:, whole]).all()      # the measurement's codes are the codec's own on whole frames
    got = op.project(other, y)
    assert got.shape == (c.B, c.L)
    want, bnd = M.expect(i.other, i.step, c.L, M.PROJECT, codes=codes)
    assert M.ratio(got.cpu().numpy(), want, bnd) <= 1.0
    again = op.project(got, y)                                     # a projected signal is consistent: it stays, up to the rounding
    Cg, Ca = M.analysis(got.cpu().numpy(), c.L).C, M.analysis(again.cpu().numpy(), c.L).C
    lo, hi, active = M.cells(ref.D, codes, c.L)
    tol = 1e-4 * np.maximum(np.abs(lo), np.abs(hi)) + 1e-5
    assert ((Cg >= lo - tol) & (Cg <= hi + tol))[active].all() and np.abs(Ca - Cg).max() <= 1e-4
    assert np.abs(Cg - M.analysis(i.other, c.L).C)[:, ~whole].max() <= 1e-4           # the edge frames are not moved
    op.noiser = P.GaussianNoise(0.01)
    with pytest.raises(ValueError, match="sigma > 0"):
        op.project(other, y)


# ---- step level -----------------------------------------------------------------------------------------------------------------------
class OracleCodec:
    """The oracle-side operator: forward = noiser(CodecSTE(x)); transform / inverse_transform are the oracle IdentityOperator's."""

    def __init__(self, step, noiser=None):
        from oracle import operators as O
        self.inner, self.noiser = O.IdentityOperator(16000), noiser
        self.step_t = torch.from_numpy(np.ascontiguousarray(np.swapaxes(np.asarray(step, np.float32), -1, -2)))

    def forward(self, data, **k):
        y = CodecSTE.apply(data, self.step_t)
        return self.noiser(y) if self.noiser is not None else y

    def transform(self, a):
        return self.inner.transform(a)

    def inverse_transform(self, mel, vocoder):
        return self.inner.inverse_transform(mel, vocoder)


class _FixedNoiser:
    def __init__(self, sigma, z):
        self.sigma, self.z = sigma, z

    def __call__(self, data):
        return data + self.sigma * self.z


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


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-300))


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.double().cpu().flatten(), b.double().cpu().flatten(), dim=0).item()


def test_forward_agrees_with_the_restatement_on_a_clip_without_ambiguous_coefficients():
    from diffmusic_amd import inverse_problem as P
    for name in M.STEP_CASES:
        c = M.CASE[name]
        i = M.inputs(c)
        assert not M.reference(c).amb.any()
        op, rop = P.CodecOperator(16000, i.step), OracleCodec(i.step)
        clean = torch.from_numpy(i.x.copy())
        rf = _rel(op.forward(clean.cuda()), rop.forward(clean))
        print(f"\n  {name}: operator.forward rel-L2 {rf:.2e}")
        assert rf < 1e-4, name


STEP_CASES = [("dps", 0.0, 5e-4, "mel_spectrogram", 501, True, 0.0), ("dps", 0.0, 5e-4, "wav_form", 996, True, 0.0),
              ("mpgd", 0.0, 5e-3, "mel_spectrogram", 251, True, 0.0), ("dsg", 1.0, 0.08, "mel_spectrogram", 501, False, 0.0),
              ("dps", 0.0, 5e-4, "mel_spectrogram", 501, True, 0.05)]


STEP_GRID_FACTOR = 0.1                 # the steps of the teacher-forced tests in units of the predicted waveform's RMS; DESIGN.md section 8.14


def _step_scale(wav_o):
    """The step grid of a teacher-forced step follows the ORACLE's predicted waveform, as the declipping test's threshold does: the grid of
    `step_test_grid` (0.5 .. 1, +inf above coefficient 256) times STEP_GRID_FACTOR times the RMS of that waveform.  The synthetic vocoder's
    level is not the 0.3 of the kernel cases, so the steps are stated relative to it.  At the factor 0.1 about 86 % of the kept codes are
    non-zero, the largest is near 480, and the vocoder's fp16 output flips 0.7 .. 0.9 % of them against the oracle's; no coarsening was
    needed for the bounds (DESIGN.md section 8.14 records factors 1, 0.1 and 0.02)."""
    return STEP_GRID_FACTOR * float(wav_o.pow(2).mean().sqrt())


def _compare(tag, sched, out, ro, name, extra=""):
    rp, rl = _rel(out.prev_sample, ro.prev_sample), _rel(out.loss.reshape(-1), ro.loss.reshape(-1))
    cos = _cos(sched.last_grad, ro.sample)
    msg = f"{tag}: prev {rp:.2e} loss {rl:.2e} grad {_rel(sched.last_grad, ro.sample):.2e} cos {cos:.4f}{extra}"
    print("\n  " + msg)
    assert _rel(out.pred_original_sample, ro.pred_original_sample) < 1e-4 or name == "mpgd"
    assert rl < 1e-2, msg
    assert cos > 0.98, msg
    assert rp < 1e-2, msg


@pytest.mark.parametrize("name,eta,rate,space,t,per_clip,sigma", STEP_CASES,
                         ids=[f"{c[0]}-{c[3]}-{'clip' if c[5] else 'batch'}-sigma{c[6]}" for c in STEP_CASES])
def test_teacher_forced_codec_step(nets, name, eta, rate, space, t, per_clip, sigma):
    """The procedure and the bounds of tests/test_gpu_declip.py::test_teacher_forced_declipping_step: forward < 1e-4 (on the fp32 clip of
    M.STEP_CASES, which has no ambiguous coefficient), loss < 1e-2, gradient cosine > 0.98, prev_sample < 1e-2.  The vocoder's fp16 output
    flips some codes against the oracle's fp32 one; the share of differing codes is printed."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    from oracle import schedulers as OS
    voc, vae, rvoc, rvae = nets
    B = 2
    g = torch.Generator().manual_seed(77)
    clean = 0.3 * torch.sin(torch.arange(LEN) * 0.05)[None] * torch.tensor([[1.0], [0.6]]) + 0.05 * torch.randn(B, LEN, generator=g)
    x = torch.randn(B, 8, H, LAT_W, generator=g)
    e = torch.randn(B, 8, H, LAT_W, generator=g)
    z = torch.randn(B, 8, H, LAT_W, generator=g)
    z_meas, z_step = torch.randn(B, LEN, generator=g), torch.randn(B, LEN, generator=g)
    rs = OS.get_scheduler(name)(operator=None, per_clip_norm=per_clip, **SCHED)
    rs.set_timesteps(200)
    with torch.no_grad():
        _, x0 = rs.parent_step(e, t, x, 0.0, None, None)
        wav_o = rvoc(rvae.decode(x0 / VAE["scaling_factor"]).sample.squeeze(1))[:, :LEN]
    grid = M.step_test_grid(M.frames(LEN), lowpass=True) * np.float32(_step_scale(wav_o))
    op, rop = P.CodecOperator(16000, grid), OracleCodec(grid)
    with torch.no_grad():
        y_clean = rop.forward(clean)
    y_ref = y_clean + sigma * z_meas if sigma > 0 else y_clean
    y = y_ref.cuda()
    op.noiser = P.GaussianNoise(sigma)
    rop.noiser = _FixedNoiser(sigma, z_step) if sigma > 0 else None
    seen = {}
    inner = op.guidance

    def spy(wav, length, *a, **k):
        seen["wav"] = wav[:, :length].detach().clone()
        return inner(wav, length, *a, **k)
    op.guidance = spy
    sched = get_scheduler(name)(operator=op, per_clip_norm=per_clip, **SCHED)
    sched.set_timesteps(200)
    sched.debug_keep_grad = True
    rs.operator = rop
    kw = dict(eta=eta, ip_guidance_rate=rate, original_waveform_length=LEN, supervised_space=space)
    noise_kw = dict(sample_noise=z.cuda()) if name == "dsg" else dict(variance_noise=None)
    opk = dict(noise=z_step.cuda()) if sigma > 0 else {}
    out = sched.step(e.cuda(), t, x.cuda(), measurement=y, vae=vae, vocoder=voc, op_kwargs=opk, **kw, **noise_kw)
    torch.cuda.synchronize()
    ro = rs.step(e, t, x, measurement=y_ref, vae=rvae, vocoder=rvoc, **kw, **(dict(sample_noise=z) if name == "dsg" else dict(variance_noise=None)))
    q_p = op.encode(seen["wav"]).cpu()
    q_o = op.encode(wav_o.contiguous().cuda()).cpu()
    coded = q_o[:, :, :256]
    flipped = float((q_p[:, :, :256] != coded).float().mean())
    nonzero = float((coded != 0).float().mean())
    _compare(f"codec {name}/{space}/{'clip' if per_clip else 'batch'}/sigma={sigma}", sched, out, ro, name,
             f" codes differing {flipped:.4f}, non-zero codes {nonzero:.3f}, largest |code| {int(coded.abs().max())}")
    assert nonzero > 0.5, "the quantiser acts on the predicted waveform: most kept coefficients span at least one cell"


def test_teacher_forced_track_step(nets):
    """One TrackOperator(CodecOperator) step at the (3, 6400, 1600, 16000) layout of tests/test_gpu_track.py, the grid built for the
    track's length, against OracleTrack(OracleCodec)."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    from oracle import schedulers as OS
    from tests.test_gpu_track import OracleTrack, T3, R3, _clean_track
    voc, vae, rvoc, rvae = nets
    lay = P.TrackLayout(T3, LEN, R3)
    Wn = lay.num_windows
    assert Wn == 3
    clean, g = _clean_track(T3)
    x = torch.randn(Wn, 8, H, LAT_W, generator=g)
    e = torch.randn(Wn, 8, H, LAT_W, generator=g)
    rs = OS.get_scheduler("dps")(operator=None, per_clip_norm=False, **SCHED)
    rs.set_timesteps(200)
    with torch.no_grad():
        _, x0 = rs.parent_step(e, 501, x, 0.0, None, None)
        wav_o = rvoc(rvae.decode(x0 / VAE["scaling_factor"]).sample.squeeze(1))[:, :LEN]
    grid = M.step_test_grid(M.frames(T3), lowpass=True) * np.float32(_step_scale(wav_o))
    op, rop = P.CodecOperator(16000, grid), OracleCodec(grid)
    with torch.no_grad():
        y_ref = rop.forward(clean)
    y = y_ref.cuda()
    kw = dict(eta=0.0, ip_guidance_rate=5e-4, original_waveform_length=LEN, supervised_space="mel_spectrogram", variance_noise=None)
    rs.operator = OracleTrack(rop, lay)
    ro = rs.step(e, 501, x, measurement=y_ref, vae=rvae, vocoder=rvoc, **kw)
    sched = get_scheduler("dps")(operator=P.TrackOperator(op, lay), per_clip_norm=False, **SCHED)
    sched.set_timesteps(200)
    sched.debug_keep_grad = True
    out = sched.step(e.cuda(), 501, x.cuda(), measurement=y, vae=vae, vocoder=voc, **kw)
    torch.cuda.synchronize()
    assert out.loss.numel() == 1
    _compare("codec inside a track", sched, out, ro, "dps")
    assert all(float(sched.last_grad[w].abs().max()) > 0 for w in range(Wn))


def test_teacher_forced_mixture_step(nets):
    """One MixtureOperator(CodecOperator, 2) step at LEN = 6400 against OracleMixture(OracleCodec)."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    from oracle import schedulers as OS
    from tests.test_gpu_mixture import OracleMixture
    voc, vae, rvoc, rvae = nets
    K, gains = 2, (2.0, 0.5)
    g = torch.Generator().manual_seed(77)
    clean = 0.3 * torch.sin(torch.arange(LEN) * 0.05)[None] * torch.tensor([[1.0], [0.6]]) + 0.05 * torch.randn(K, LEN, generator=g)
    x = torch.randn(K, 8, H, LAT_W, generator=g)
    e = torch.randn(K, 8, H, LAT_W, generator=g)
    rs = OS.get_scheduler("dps")(operator=None, per_clip_norm=False, **SCHED)
    rs.set_timesteps(200)
    with torch.no_grad():
        _, x0 = rs.parent_step(e, 501, x, 0.0, None, None)
        wav_o = rvoc(rvae.decode(x0 / VAE["scaling_factor"]).sample.squeeze(1))[:, :LEN]
    grid = M.step_test_grid(M.frames(LEN), lowpass=True) * np.float32(_step_scale(wav_o))
    op, rop = P.CodecOperator(16000, grid), OracleCodec(grid)
    top, rtop = P.MixtureOperator(op, K, list(gains)), OracleMixture(rop, gains)
    with torch.no_grad():
        y_ref = rtop.forward(clean)
    assert y_ref.shape[0] == 1
    y = y_ref.cuda()
    kw = dict(eta=0.0, ip_guidance_rate=5e-4, original_waveform_length=LEN, supervised_space="mel_spectrogram", variance_noise=None)
    rs.operator = rtop
    ro = rs.step(e, 501, x, measurement=y_ref, vae=rvae, vocoder=rvoc, **kw)
    sched = get_scheduler("dps")(operator=top, per_clip_norm=False, **SCHED)
    sched.set_timesteps(200)
    sched.debug_keep_grad = True
    out = sched.step(e.cuda(), 501, x.cuda(), measurement=y, vae=vae, vocoder=voc, **kw)
    torch.cuda.synchronize()
    assert out.loss.numel() == 1
    _compare("codec inside a mixture", sched, out, ro, "dps")
    assert all(float(sched.last_grad[k].abs().max()) > 0 for k in range(K))


# ---- call level -----------------------------------------------------------------------------------------------------------------------
SECONDS = 0.4


def _clips(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.arange(T, dtype=torch.float32)
    return (0.3 * torch.sin(n * 0.05)[None] * torch.linspace(1.0, 0.6, B)[:, None] * (1.0 + 0.3 * torch.sin(n * 0.0007))[None]
            + 0.05 * torch.randn(B, T, generator=g)).cuda().contiguous()


def _problem(B, T, seed=11):
    g = torch.Generator().manual_seed(seed)
    pe = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    return pe, _clips(B, T, seed)


def _nmr_grid(clean, nmr_db=12.0, cutoff_hz=6000.0):
    from diffmusic_amd import inverse_problem as P
    return P.codec_steps_for_nmr(clean.cpu().numpy(), 16000, nmr_db, cutoff_hz=cutoff_hz)


def test_call_equals_the_hand_written_loop(monkeypatch):
    """`pipe(...)` with a CodecOperator (signal-adaptive per-clip grids) against `_unet_eps` + `scheduler.step` written out: bit for bit,
    latents and losses; the ctypes binding gives the same bits; per-clip grids are refused under lanes by name; `project` on the result."""
    from diffmusic_amd import inverse_problem as P, ops
    from tests.test_gpu_declip import _pipe, _gens, _hand_loop, N_CALL
    B = 3
    pe, clean = _problem(B, LEN)
    op = P.CodecOperator(16000, _nmr_grid(clean), noiser=P.GaussianNoise(0.0))
    assert op.per_clip and not op.lossless
    pipe = _pipe(op)
    y = op.forward(clean)
    assert float((y - clean).abs().max()) > 0.01                  # the codec acts
    call = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0)
    got = pipe(generator=_gens(B), output_type="latent", **call).audios
    assert len(pipe.last_losses) == N_CALL and pipe.nan_restarts == 0
    got_losses = [l.reshape(-1).clone() for l in pipe.last_losses]
    x, losses = _hand_loop(pipe, pe, y, B)
    assert torch.equal(got, x)
    assert all(torch.equal(a, b.reshape(-1)) for a, b in zip(got_losses, losses))
    assert all(bool(torch.isfinite(l).all()) and bool((l > 0).all()) for l in got_losses)
    monkeypatch.setattr(ops, "USE_TORCH_OPS", False)
    assert not ops.enabled()
    y_ct = op.forward(clean)
    got_ct = pipe(generator=_gens(B), output_type="latent", **call).audios
    monkeypatch.setattr(ops, "USE_TORCH_OPS", True)
    assert torch.equal(y, y_ct) and torch.equal(got, got_ct)
    with pytest.raises(ValueError, match="per-clip step grids cannot run as clip lanes"):
        pipe(generator=_gens(B), output_type="latent", lanes=2, **call)
    # the opt-in output stage on the decoded audio: whole frames end up in the cells of the measurement's codes
    audio = pipe(generator=_gens(B), output_type="pt", **call).audios
    assert audio.shape == (B, LEN)
    proj = op.project(audio, y)
    assert proj.shape == (B, LEN) and bool(torch.isfinite(proj).all())
    codes = op.encode(y).cpu().numpy().astype(np.int64)
    D = M.step_btk(op.step.numpy(), B)
    lo, hi, active = M.cells(D, codes, LEN)
    Cp = M.analysis(proj.cpu().numpy(), LEN).C
    tol = 1e-4 * np.maximum(np.abs(lo), np.abs(hi)) + 1e-5
    assert active.any() and ((Cp >= lo - tol) & (Cp <= hi + tol))[active].all()


def test_inside_a_track_equals_its_hand_loop():
    from diffmusic_amd import inverse_problem as P
    from tests.test_gpu_declip import _pipe, _gens, _hand_loop, N_CALL
    T, R = 16000, 1600                                       # windows of 6400 at 0, 4800, 9600
    lay = P.TrackLayout(T, LEN, R)
    assert lay.num_windows == 3
    pe, clean = _problem(3, T, seed=21)
    clean = clean[:1].contiguous()
    inner = P.CodecOperator(16000, _nmr_grid(clean[0]), noiser=P.GaussianNoise(0.0))         # the grid is built for the track's length
    assert tuple(inner.step.shape) == (512, M.frames(T))
    top = P.TrackOperator(inner, lay)
    pipe = _pipe(top, per_clip=False)
    y = top.forward(clean)
    assert y.shape == (1, T) and float((y - clean).abs().max()) > 0.01
    call = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0)
    lat = pipe(generator=_gens(3), output_type="latent", **call).audios
    assert lat.shape == (3, 8, 10, 16) and len(pipe.last_losses) == N_CALL and all(l.numel() == 1 for l in pipe.last_losses)
    call_losses = [l.reshape(-1).clone() for l in pipe.last_losses]
    x, losses = _hand_loop(pipe, pe, y, 3)
    assert torch.equal(lat, x)
    assert all(torch.equal(a, b.reshape(-1)) for a, b in zip(call_losses, losses))
    assert all(bool(torch.isfinite(l).all()) and bool((l > 0).all()) for l in call_losses)


def test_inside_a_mixture_equals_its_hand_loop():
    from diffmusic_amd import inverse_problem as P
    from tests.test_gpu_mixture import _pipe, _gens, _hand_loop, N_CALL
    K = 2
    pe, clean = _problem(K, LEN, seed=31)
    mix = (clean[0] + 0.5 * clean[1])
    inner = P.CodecOperator(16000, _nmr_grid(mix), noiser=P.GaussianNoise(0.0))
    top = P.MixtureOperator(inner, K, [1.0, 0.5])
    pipe = _pipe(top)
    y = top.forward(clean)
    assert y.shape == (1, LEN)                                    # the codec acts on the mix
    call = dict(prompt_embeds=pe, audio_length_in_s=SECONDS, num_inference_steps=N_CALL, show_progress=False, measurement=y, eta=0.0)
    lat = pipe(generator=_gens(K), output_type="latent", **call).audios
    assert len(pipe.last_losses) == N_CALL and all(l.numel() == 1 for l in pipe.last_losses)
    got_losses = list(pipe.last_losses)
    _, x, losses = _hand_loop(pipe, pe, y, K)
    assert torch.equal(lat, x)
    assert all(torch.equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(got_losses, losses))
    assert all(bool(torch.isfinite(l).all()) and bool((l > 0).all()) for l in got_losses)


def test_clip_lanes_with_a_shared_grid_equal_the_plain_loop():
    """lanes = 2 on four clips equals the two clip groups run with lanes = 1, bit for bit (a shared grid is no per-clip state), the
    procedure of tests/test_gpu_lanes.py on the small nets; `shard=True` refuses per-clip grids by name."""
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.pipelines.lanes import split_sizes
    from diffmusic_amd.pipelines.pipeline_musicldm import MusicLDMPipeline
    from tests.test_gpu_pipeline import UNET, _build
    B, N = 4, 4
    grid = P.codec_step_grid(LEN, 16000, -26.0, cutoff_hz=6000.0, tilt_db_per_octave=3.0)
    op = P.CodecOperator(16000, grid, noiser=P.GaussianNoise(0.0))
    assert op.positional_state is None
    pipe = _build("musicldm", UNET, "dps", op)
    g = torch.Generator().manual_seed(3)
    pe = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    ne = torch.nn.functional.normalize(torch.randn(B, 512, generator=g), dim=-1)
    lat0 = torch.randn(B, 8, 10, 16, generator=g)
    y = op.forward(_clips(B, LEN, 3))

    def call(ids, lanes):
        gens = [torch.Generator().manual_seed(100 + k) for k in ids]
        out = pipe(prompt_embeds=pe[ids], negative_prompt_embeds=ne[ids], audio_length_in_s=SECONDS, num_inference_steps=N, guidance_scale=2.0,
                   latents=lat0[ids].clone(), measurement=y[ids].contiguous(), ip_guidance_rate=5e-4, eta=0.0, generator=gens,
                   show_progress=False, output_type="latent", lanes=lanes)
        return out.audios, [l.reshape(-1).clone() for l in pipe.last_losses]
    got, losses = call(list(range(B)), 2)
    assert got.shape == (B, 8, 10, 16) and len(losses) == N
    o = 0
    for n in split_sizes(B, 2):
        ids = list(range(o, o + n))
        ref, ref_losses = call(ids, 1)
        assert torch.equal(got[ids], ref), f"lane {ids}: latents differ from the plain loop on those clips"
        assert all(torch.equal(losses[k][ids], ref_losses[k]) for k in range(N)), f"lane {ids}: a loss differs"
        o += n
    pipe.scheduler.operator = P.CodecOperator(16000, np.stack([grid] * B))
    with pytest.raises(ValueError, match="per-clip step grids cannot be sharded|step grids.*shard|shard.*step grids"):
        MusicLDMPipeline._check_positional_state(pipe, True, None, None)
    with pytest.raises(ValueError, match="per-clip step grids cannot run as clip lanes"):
        MusicLDMPipeline._check_positional_state(pipe, False, None, 2)
