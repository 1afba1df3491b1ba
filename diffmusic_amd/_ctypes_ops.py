"""The ctypes spelling of the op surface: one function per op registered in csrc_torch/torch_ops.cpp, with the op's name, parameters
(names, order, positional / keyword-only split, defaults), return values, dtypes and shapes, over the same `extern "C"` launchers of
libdiffmusic_hip.so (`_lib.py`).  Outputs come from torch's caching allocator, launches go to torch's current HIP stream, model /
audio handles arrive as Python ints.

`ops.hip.<name>` resolves here when the op library is switched off or unavailable (ops.py); `ops.ctypes_hip` is this module.  There
is one function per operation: what it can do beyond its plain form (caller-owned outputs with their row strides, prediction type and
clip range, measurement noise and clip thresholds of the guidance pair, a dead span, context tensors, a U-Net whose output channels
differ from its input's) is a defaulted parameter, and the function calls the longest rung of the C ABI's additive ladder
(_ex / _shaped / _ctx / _dead), which stays for C callers.  tests/test_abi.py holds every signature equal to its schema."""
import ctypes as C

import torch

from . import _lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def abi_version():
    return _lib.lib().dmx_abi_version()


# ---- scheduler arithmetic
def sched_pred_x0(x, eps, alpha_t, *, ptype=0, clip_r=0.0):
    """ptype / clip_r: the DDIM parent's other branches (sample / v_prediction, clip_sample), the `_ex` entry point."""
    x0 = torch.empty_like(x)
    if ptype == 0 and clip_r == 0.0:
        _lib.check(_lib.lib().dmx_sched_pred_x0(_p(x), _p(eps), _p(x0), x.numel(), alpha_t, _stream()), "pred_x0")
    else:
        _lib.check(_lib.lib().dmx_sched_pred_x0_ex(_p(x), _p(eps), _p(x0), x.numel(), alpha_t, ptype, clip_r, _stream()), "pred_x0_ex")
    return x0


def cfg_combine(eps2, scale):
    out = torch.empty_like(eps2[:eps2.shape[0] // 2])           # the [uncond | text] halves of the CFG batch -> one half
    _lib.check(_lib.lib().dmx_sched_cfg_combine(_p(eps2), _p(out), out.numel(), scale, _stream()), "cfg_combine")
    return out


def sched_update(mode, x, eps, x0, g0, inv_scale, noise, alpha_t, alpha_prev, sigma, rate, eps_small, global_norm, *,
                 ptype=0, clip_r=0.0, grad_out=None):
    """-> (prev_sample, MPGD's guided x0 or None).  grad_out: caller-owned tensor like x that receives the applied gradient."""
    B, n = x.shape[0], x[0].numel()
    prev = torch.empty_like(x)
    x0_out = torch.empty_like(x) if mode == 2 else None
    if ptype == 0 and clip_r == 0.0:
        _lib.check(_lib.lib().dmx_sched_step(mode, _p(x), _p(eps), _p(x0), _p(g0), _p(inv_scale), _p(noise), _p(prev), _p(x0_out),
                                             _p(grad_out), B, n, alpha_t, alpha_prev, sigma, rate, eps_small, int(global_norm),
                                             _stream()), "sched_step")
    else:
        _lib.check(_lib.lib().dmx_sched_step_ex(mode, _p(x), _p(eps), _p(x0), _p(g0), _p(inv_scale), _p(noise), _p(prev), _p(x0_out),
                                                _p(grad_out), B, n, alpha_t, alpha_prev, sigma, rate, eps_small, int(global_norm),
                                                ptype, clip_r, _stream()), "sched_step_ex")
    return prev, x0_out


def randn_philox(shape, seeds, offset, device):
    """Seeds and offset are taken modulo 2^64 (the op's ints are signed 64-bit: `torch_utils.randn_philox` folds larger values)."""
    B = int(shape[0])
    n = 1
    for d in shape[1:]:
        n *= int(d)
    out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    arr = (C.c_ulonglong * B)(*[int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds])
    _lib.check(_lib.lib().dmx_randn_philox(_p(out), B, n, arr, int(offset) & 0xFFFFFFFFFFFFFFFF, _stream()), "randn_philox")
    return out


# ---- measurement operators and the loss
def mask_mul(x, mask, L, Ly):
    """y[:, :L] = x[:, :L] * mask (None: copy), zeros up to Ly; x (B, >= L) with any row stride."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1, ("mask_mul", x.shape)
    assert mask is None or (mask.dtype == torch.float32 and mask.is_contiguous()), "mask_mul: mask must be contiguous fp32"
    B = x.shape[0]
    y = torch.empty(B, Ly, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dmx_mask_apply(_p(x), x.stride(0), _p(mask), _p(y), Ly, B, L, Ly, _stream()), "mask_mul")
    return y


def l2norm(ref, pred, gscale, *, want_grad=True):
    """-> (loss (B), dpred like pred, or None when want_grad is False); ref and pred contiguous."""
    assert ref.is_contiguous() and pred.is_contiguous(), ("l2norm", ref.shape, pred.shape)
    B = pred.shape[0]
    n = pred[0].numel()
    loss = torch.empty(B, dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    _lib.check(_lib.lib().dmx_l2_loss(_p(ref), 0 if ref.shape[0] == 1 and B > 1 else n, _p(pred), _p(loss), _p(dpred), B, n, gscale,
                                      _stream()), "l2_loss")
    return loss, dpred


def resample_fwd(x, h, Lin, Lout, orig, new_, off):
    B = x.shape[0]
    y = torch.empty(B, Lout, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dmx_fir_fwd(_p(x), x.stride(0), _p(h), _p(y), Lout, B, Lin, Lout, h.shape[-1], orig, new_, off, _stream()),
               "fir_fwd")
    return y


def resample_bwd(dy, h, h_rev, Lin, Lfull, orig, new_, off):
    B, out_len = dy.shape
    d = torch.zeros(B, Lfull, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().dmx_fir_bwd(_p(dy), out_len, _p(h), _p(h_rev), _p(d), Lfull, B, Lin, out_len, h.shape[-1], orig, new_, off,
                                      _stream()), "fir_bwd")
    return d


def _rows(name, x, L):
    if not x.is_cuda:
        raise RuntimeError(f"{name}: tensors must be on the GPU (no CPU fallback)")
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] >= L >= 1, (name, x.shape, L)


def _taps(name, h, B):
    assert h.is_cuda and h.dtype == torch.float32 and h.dim() == 2 and h.is_contiguous() and h.shape[0] == B and h.shape[1] >= 1, \
        (name, h.shape, B)
    return h.shape[1]


def fir_clip_fwd(x, h, Lin):
    """x (B, >= Lin) with any row stride, h (B, n) one response per clip -> (B, Lin + 2 * (n // 2) - n + 1): conv1d with padding n // 2."""
    _rows("fir_clip_fwd", x, Lin)
    B = x.shape[0]
    n = _taps("fir_clip_fwd", h, B)
    Lout = Lin + 2 * (n // 2) - n + 1
    y = torch.empty(B, Lout, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dmx_fir_clip_fwd(_p(x), x.stride(0), _p(h), _p(y), Lout, B, Lin, Lout, n, _stream()), "fir_clip_fwd")
    return y


def fir_clip_bwd(dy, h, h_rev, Lin, Lfull):
    """The transpose in x: dy (B, Lout) contiguous, h and its time reverse h_rev (B, n) -> (B, Lfull), zeros past Lin."""
    _rows("fir_clip_bwd", dy, dy.shape[1] if dy.dim() == 2 else 1)
    B, Lout = dy.shape
    n = _taps("fir_clip_bwd", h, B)
    assert _taps("fir_clip_bwd", h_rev, B) == n and dy.is_contiguous() and Lfull >= Lin >= 1 and Lout == Lin + 2 * (n // 2) - n + 1, \
        (dy.shape, h.shape, h_rev.shape, Lin, Lfull)
    d = torch.zeros(B, Lfull, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().dmx_fir_clip_bwd(_p(dy), Lout, _p(h), _p(h_rev), _p(d), Lfull, B, Lin, Lout, n, _stream()), "fir_clip_bwd")
    return d


def fir_wgrad(dy, x, L, taps):
    """The gradient in h as partial sums: dy (B, Lout) contiguous, x (B, >= L) with any row stride -> (B, segments, taps); row s holds the
    terms of outputs [4096 s, 4096 (s + 1)), dh = the sum over s (`ir_update` adds the rows in order)."""
    _rows("fir_wgrad", x, L)
    _rows("fir_wgrad", dy, dy.shape[1] if dy.dim() == 2 else 1)
    B, Lout = dy.shape
    assert x.shape[0] == B and dy.is_contiguous() and taps >= 1 and Lout == L + 2 * (taps // 2) - taps + 1, (dy.shape, x.shape, L, taps)
    lib = _lib.lib()
    segments = lib.dmx_fir_wgrad_workspace_floats(B, Lout, taps) // (B * taps)
    part = torch.empty(B, segments, taps, dtype=torch.float32, device=dy.device)
    _lib.check(lib.dmx_fir_wgrad(_p(dy), Lout, _p(x), x.stride(0), _p(part), part.numel(), B, L, Lout, taps, _stream()), "fir_wgrad")
    return part


def ir_update(partials, h, h_rev, m, v, k, lr, beta1, beta2, eps):
    """One Adam step on the responses from the partial rows of `fir_wgrad`, then h <- h' / max|h'| per clip; h, h_rev, m, v (B, n) are
    updated IN PLACE, k is the 1-based count of updates since the last reset.  A clip whose gradient or step is not finite keeps its
    state."""
    assert partials.is_cuda and partials.dtype == torch.float32 and partials.dim() == 3 and partials.is_contiguous(), partials.shape
    B, segments, n = partials.shape
    for t in (h, h_rev, m, v):
        assert _taps("ir_update", t, B) == n, (t.shape, partials.shape)
    _lib.check(_lib.lib().dmx_ir_update(_p(partials), segments, _p(h), _p(h_rev), _p(m), _p(v), B, n, float(lr), float(beta1), float(beta2),
                                        float(eps), int(k), _stream()), "ir_update")


def logmel_fwd(audio, wav, state, L, power2, to_db, lo, hi, *, out=None):
    """out: caller-owned contiguous (B, frames, 64) result."""
    lib = _lib.lib()
    B, T = wav.shape[0], lib.dmx_audio_num_frames(audio, L)
    assert out is None or (out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * T * 64), ("logmel_fwd", out.shape)
    mel = out if out is not None else torch.empty(B, T, 64, dtype=torch.float32, device=wav.device)
    _lib.check(lib.dmx_audio_transform_fwd(audio, _p(wav), wav.stride(0), _p(mel), _p(state), B, L, int(power2), int(to_db), lo, hi,
                                           _stream()), "audio_transform_fwd")
    return mel


def logmel_bwd(audio, dmel, state, L, power2, to_db, lo, hi, *, dwav=None):
    """dwav: caller-owned (B, >= L) result with any row stride (overwritten up to L)."""
    B = dmel.shape[0]
    if dwav is None:
        dwav = torch.empty(B, L, dtype=torch.float32, device=dmel.device)
    else:
        _rows("logmel_bwd", dwav, L)
    _lib.check(_lib.lib().dmx_audio_transform_bwd(audio, _p(dmel), _p(dwav), dwav.stride(0), _p(state), B, L, int(power2), int(to_db),
                                                  lo, hi, 0, _stream()), "audio_transform_bwd")
    return dwav


def mel_guidance(audio, wav, mask, ref, state, L, Lfull, power2, to_db, lo, hi, gscale, noise=None, noise_mag=None, sigma=0.0, thr=None):
    """The fused guidance pair -> (loss (B), dwav (B, Lfull)).  The step's measurement noise: noise (B, >= L) in the sample domain and / or
    noise_mag (B, bins, frames) on the magnitudes (power2 False only), standard-normal draws used as sigma * noise.  thr (B) fp32: per-clip
    hard-clip thresholds c > 0 between the mask and the noise, y = clip(wav * mask, c) + sigma * noise, gradient through
    -c <= wav * mask <= c only."""
    lib = _lib.lib()
    B = wav.shape[0]
    T = lib.dmx_audio_num_frames(audio, L)
    assert ref.numel() in (T * 64, B * T * 64), (ref.shape, B, T)
    assert noise is None or (noise.shape[0] == B and noise.shape[1] >= L and noise.stride(1) == 1), noise.shape
    assert noise_mag is None or (noise_mag.is_contiguous() and noise_mag.numel() == B * lib.dmx_audio_num_bins(audio) * T), noise_mag.shape
    assert thr is None or (thr.is_cuda and thr.dtype == torch.float32 and thr.is_contiguous() and thr.numel() == B), (thr.shape, B)
    rs = 0 if (ref.numel() == T * 64 and B > 1) else T * 64
    ns = noise.stride(0) if noise is not None else 0
    loss = torch.empty(B, dtype=torch.float32, device=wav.device)
    dwav = torch.empty(B, Lfull, dtype=torch.float32, device=wav.device)
    _lib.check(lib.dmx_audio_guidance_fwd_shaped(audio, _p(wav), wav.stride(0), _p(mask), _p(ref), rs, None, _p(state), B, L, int(power2),
                                                 int(to_db), lo, hi, _p(noise), ns, _p(noise_mag), sigma, _p(thr), _stream()),
               "audio_guidance_fwd_shaped")
    _lib.check(lib.dmx_audio_guidance_bwd_shaped(audio, _p(wav), wav.stride(0), _p(mask), _p(ref), rs, gscale, _p(loss), _p(dwav), Lfull, Lfull,
                                                 _p(state), B, L, int(power2), int(to_db), lo, hi, _p(noise), ns, _p(noise_mag), sigma, _p(thr),
                                                 _stream()), "audio_guidance_bwd_shaped")
    return loss, dwav


def _clip_args(name, x, thr, L):
    if not x.is_cuda:
        raise RuntimeError(f"{name}: tensors must be on the GPU (no CPU fallback)")
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] >= L >= 1, (name, x.shape, L)
    assert thr.is_cuda and thr.dtype == torch.float32 and thr.is_contiguous() and thr.numel() == x.shape[0], (name, thr.shape, x.shape)


def clip_fwd(x, thr, L):
    """x (B, >= L) with any row stride, thr (B) -> contiguous (B, L): min(max(x, -thr[b]), thr[b]); a NaN stays NaN."""
    _clip_args("clip_fwd", x, thr, L)
    B = x.shape[0]
    y = torch.empty(B, L, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dmx_clip_fwd(_p(x), x.stride(0), _p(thr), _p(y), L, B, L, _stream()), "clip_fwd")
    return y


def clip_bwd(dy, wav, thr, Lfull):
    """dy (B, L) contiguous, wav (B, >= L) with any row stride -> (B, Lfull): dy where -thr[b] <= wav <= thr[b], zero elsewhere and past L."""
    assert dy.dtype == torch.float32 and dy.dim() == 2 and dy.is_contiguous() and Lfull >= dy.shape[1], (dy.shape, Lfull)
    B, L = dy.shape
    _clip_args("clip_bwd", wav, thr, L)
    assert wav.shape[0] == B and dy.is_cuda, (wav.shape, dy.shape)
    d = torch.empty(B, Lfull, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().dmx_clip_bwd(_p(dy), L, _p(wav), wav.stride(0), _p(thr), _p(d), Lfull, B, L, Lfull, _stream()), "clip_bwd")
    return d


def declip_project(wav, measurement, thr, L):
    """wav (B, >= L) restored, measurement (B, >= L) clipped at thr (B) -> contiguous (B, L): the measurement where |y| < c, else the
    restored sample pushed to the clipped side (max(wav, c) for y >= c, min(wav, -c) for y <= -c)."""
    _clip_args("declip_project", wav, thr, L)
    _clip_args("declip_project", measurement, thr, L)
    B = wav.shape[0]
    out = torch.empty(B, L, dtype=torch.float32, device=wav.device)
    _lib.check(_lib.lib().dmx_declip_project(_p(wav), wav.stride(0), _p(measurement), measurement.stride(0), _p(thr), _p(out), L, B, L, _stream()),
               "declip_project")
    return out


def drc_fwd(x, L, threshold_db, slope, knee_db, a_att, a_rel, makeup_db):
    """x (B, >= L) with any row stride -> (y (B, L), state (B, 3, H) fp32 with the rows p, G, s, tape (B, H) uint8: bits 0-1 the region of
    the static curve, bit 2 the attack gate), H = ceil(L / 64): the block-rate compressor of csrc/drc.hip.  slope = 1 - 1 / ratio."""
    if not x.is_cuda:
        raise RuntimeError("drc_fwd: tensors must be on the GPU (no CPU fallback)")
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] >= L >= 1, ("drc_fwd", x.shape, L)
    B, H = x.shape[0], -(-L // 64)
    y = torch.empty(B, L, dtype=torch.float32, device=x.device)
    state = torch.empty(B, 3, H, dtype=torch.float32, device=x.device)
    tape = torch.empty(B, H, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().dmx_drc_fwd(_p(x), x.stride(0), _p(y), L, _p(state), _p(tape), min(B, 65536), L, threshold_db, slope, knee_db, a_att,
                                      a_rel, makeup_db, _stream()), "drc_fwd")
    return y, state, tape


def drc_bwd(dy, x, state, tape, Lfull, threshold_db, slope, knee_db, a_att, a_rel, makeup_db):
    """dy (B, L) and x (B, >= L) with any row strides, state and tape as `drc_fwd` returned them for x -> (B, Lfull): the transpose of the
    Jacobian of drc_fwd at x applied to dy, zeros past L.  The gates come from the tape."""
    if not dy.is_cuda:
        raise RuntimeError("drc_bwd: tensors must be on the GPU (no CPU fallback)")
    assert dy.dtype == torch.float32 and dy.dim() == 2 and dy.stride(1) == 1 and Lfull >= dy.shape[1] >= 1, ("drc_bwd", dy.shape, Lfull)
    B, L = dy.shape
    H = -(-L // 64)
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == B and x.shape[1] >= L and \
        x.device == dy.device, ("drc_bwd", x.shape, dy.shape)
    assert state.device == dy.device and state.dtype == torch.float32 and state.is_contiguous() and tuple(state.shape) == (B, 3, H), \
        ("drc_bwd", tuple(state.shape), (B, 3, H))
    assert tape.device == dy.device and tape.dtype == torch.uint8 and tape.is_contiguous() and tuple(tape.shape) == (B, H), \
        ("drc_bwd", tuple(tape.shape), (B, H))
    work = torch.empty(B, H, dtype=torch.float32, device=dy.device)
    d = torch.empty(B, Lfull, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().dmx_drc_bwd(_p(dy), dy.stride(0), _p(x), x.stride(0), _p(state), _p(tape), _p(work), _p(d), Lfull, min(B, 65536), L, Lfull,
                                      threshold_db, slope, knee_db, a_att, a_rel, makeup_db, _stream()), "drc_bwd")
    return d


def _drc_table(who, theta, B, like):
    assert theta.is_cuda and theta.device == like.device and theta.dtype == torch.float32 and theta.is_contiguous() and \
        tuple(theta.shape) == (B, 8), (who, tuple(theta.shape), (B, 8))


def _drc_tape(who, state, tape, B, H, like):
    assert state.is_cuda and state.device == like.device and state.dtype == torch.float32 and state.is_contiguous() and \
        tuple(state.shape) == (B, 3, H), (who, tuple(state.shape), (B, 3, H))
    assert tape.is_cuda and tape.device == like.device and tape.dtype == torch.uint8 and tape.is_contiguous() and tuple(tape.shape) == (B, H), \
        (who, tuple(tape.shape), (B, H))


def drc_fwd_p(x, L, theta, knee_db):
    """`drc_fwd` with the parameters of clip b read from theta[b] on the device: theta (B, 8) fp32, rows T, k, makeup, aA, aR, 1 - aA, 1 - aR,
    k / (2 knee_db) (`dsp.drc_table` builds one).  -> (y, state, tape) as `drc_fwd`, bit-equal to it on a table of equal rows."""
    if not x.is_cuda:
        raise RuntimeError("drc_fwd_p: tensors must be on the GPU (no CPU fallback)")
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] >= L >= 1, ("drc_fwd_p", x.shape, L)
    B, H = x.shape[0], -(-L // 64)
    _drc_table("drc_fwd_p", theta, B, x)
    y = torch.empty(B, L, dtype=torch.float32, device=x.device)
    state = torch.empty(B, 3, H, dtype=torch.float32, device=x.device)
    tape = torch.empty(B, H, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().dmx_drc_fwd_p(_p(x), x.stride(0), _p(y), L, _p(state), _p(tape), _p(theta), min(B, 65536), L, knee_db, _stream()),
               "drc_fwd_p")
    return y, state, tape


def drc_bwd_p(dy, x, state, tape, theta, Lfull, knee_db):
    """`drc_bwd` with the table of `drc_fwd_p` -> (dx (B, Lfull), work (B, 2, H): rows ds and dc, bq0 (B,): Bq[0] of each clip) -- what
    `drc_pgrad` needs besides the state and the tape."""
    if not dy.is_cuda:
        raise RuntimeError("drc_bwd_p: tensors must be on the GPU (no CPU fallback)")
    assert dy.dtype == torch.float32 and dy.dim() == 2 and dy.stride(1) == 1 and Lfull >= dy.shape[1] >= 1, ("drc_bwd_p", dy.shape, Lfull)
    B, L = dy.shape
    H = -(-L // 64)
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == B and x.shape[1] >= L and \
        x.device == dy.device, ("drc_bwd_p", x.shape, dy.shape)
    _drc_tape("drc_bwd_p", state, tape, B, H, dy)
    _drc_table("drc_bwd_p", theta, B, dy)
    work = torch.empty(B, 2, H, dtype=torch.float32, device=dy.device)
    bq0 = torch.empty(B, dtype=torch.float32, device=dy.device)
    d = torch.empty(B, Lfull, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().dmx_drc_bwd_p(_p(dy), dy.stride(0), _p(x), x.stride(0), _p(state), _p(tape), _p(theta), _p(work), _p(bq0), _p(d), Lfull,
                                        min(B, 65536), L, Lfull, knee_db, _stream()), "drc_bwd_p")
    return d, work, bq0


def drc_pgrad(state, tape, work, bq0, theta, L, knee_db):
    """state and tape of `drc_fwd_p`, work and bq0 of `drc_bwd_p` -> part (B, ceil(H / 256), 5): the gradient of the loss in (T, k, makeup,
    ln aA, ln aR) as one row per segment of 256 blocks; the gradient is the sum over the segments (csrc/drc_fit.hip)."""
    if not work.is_cuda:
        raise RuntimeError("drc_pgrad: tensors must be on the GPU (no CPU fallback)")
    assert 1 <= L <= 1 << 30, ("drc_pgrad", L)
    H = -(-L // 64)
    assert work.dtype == torch.float32 and work.dim() == 3 and work.is_contiguous() and work.shape[0] >= 1 and tuple(work.shape[1:]) == (2, H), \
        ("drc_pgrad", tuple(work.shape), (2, H))
    B = work.shape[0]
    _drc_tape("drc_pgrad", state, tape, B, H, work)
    _drc_table("drc_pgrad", theta, B, work)
    assert bq0.is_cuda and bq0.device == work.device and bq0.dtype == torch.float32 and bq0.is_contiguous() and tuple(bq0.shape) == (B,), \
        ("drc_pgrad", tuple(bq0.shape), (B,))
    part = torch.empty(B, -(-H // 256), 5, dtype=torch.float32, device=work.device)
    _lib.check(_lib.lib().dmx_drc_pgrad(_p(state), _p(tape), _p(work), _p(bq0), _p(theta), _p(part), min(B, 65536), L, knee_db, _stream()),
               "drc_pgrad")
    return part


def drc_update(part, phi, m, v, theta, L, k, lr, beta1, beta2, eps, knee_db, lo, hi):
    """One Adam step per parameter on phi = (T, k, makeup, ln aA, ln aR) from the rows of `drc_pgrad`, with its own lr[q] (0 freezes it), the
    clamp to [lo[q], hi[q]] and the clip's new row of theta; phi, m, v (B, 5) and theta (B, 8) are updated IN PLACE, k the 1-based count of
    updates since the last reset.  A clip whose gradient or step is not finite keeps its state."""
    if not part.is_cuda:
        raise RuntimeError("drc_update: tensors must be on the GPU (no CPU fallback)")
    assert 1 <= L <= 1 << 30 and len(lr) == 5 and len(lo) == 5 and len(hi) == 5, ("drc_update", L, lr, lo, hi)
    H = -(-L // 64)
    assert part.dtype == torch.float32 and part.dim() == 3 and part.is_contiguous() and part.shape[0] >= 1 and \
        tuple(part.shape[1:]) == (-(-H // 256), 5), ("drc_update", tuple(part.shape), (-(-H // 256), 5))
    B = part.shape[0]
    for t in (phi, m, v):
        assert t.is_cuda and t.device == part.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, 5), \
            ("drc_update", tuple(t.shape), (B, 5))
    _drc_table("drc_update", theta, B, part)
    five = C.c_double * 5
    _lib.check(_lib.lib().dmx_drc_update(_p(part), _p(phi), _p(m), _p(v), _p(theta), B, L, int(k), five(*[float(a) for a in lr]), float(beta1),
                                         float(beta2), float(eps), float(knee_db), five(*[float(a) for a in lo]),
                                         five(*[float(a) for a in hi]), _stream()), "drc_update")


def _warp_delay_stride(who, delay, like, B, length):
    K = -(-length // 64) + 1
    assert delay.is_cuda and delay.device == like.device and delay.dtype == torch.float32 and delay.is_contiguous() and \
        tuple(delay.shape) in ((K,), (B, K)), (who, tuple(delay.shape), "expected", (K,), "or", (B, K))
    return 0 if delay.dim() == 1 else K


def warp_fwd(x, delay, length):
    """x (B, >= length) with any row stride, delay (H + 1) for every clip or (B, H + 1), H = ceil(length / 64), contiguous fp32 knots in
    samples -> (B, length): the clip read along the delay curve, four-point Catmull-Rom (csrc/warp.hip)."""
    if not x.is_cuda:
        raise RuntimeError("warp_fwd: tensors must be on the GPU (no CPU fallback)")
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] >= length >= 1 and length <= 1 << 30, \
        ("warp_fwd", x.shape, length)
    B = x.shape[0]
    ds = _warp_delay_stride("warp_fwd", delay, x, B, length)
    y = torch.empty(B, length, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dmx_warp_fwd(_p(x), x.stride(0), _p(delay), ds, _p(y), min(B, 65536), length, _stream()), "warp_fwd")
    return y


def warp_bwd(dy, delay, length, full):
    """dy (B, length) contiguous, delay as for `warp_fwd` -> (B, full): the transpose of `warp_fwd` applied to dy, a gather without atomics,
    zeros past `length`."""
    if not dy.is_cuda:
        raise RuntimeError("warp_bwd: tensors must be on the GPU (no CPU fallback)")
    assert dy.dtype == torch.float32 and dy.dim() == 2 and dy.is_contiguous() and dy.shape[1] == length >= 1 and length <= full <= 1 << 30, \
        ("warp_bwd", dy.shape, length, full)
    B = dy.shape[0]
    ds = _warp_delay_stride("warp_bwd", delay, dy, B, length)
    d = torch.empty(B, full, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().dmx_warp_bwd(_p(dy), _p(delay), ds, _p(d), min(B, 65536), length, full, _stream()), "warp_bwd")
    return d


def warp_wgrad(dy, x, delay, length):
    """dy = dLoss/dy (B, length) contiguous, x (B, >= length) with any row stride, delay as for `warp_fwd` -> part (B, H, 2): the gradient of
    the loss in the fine knots as one pair per block of 64 samples, dd[j] = part[:, j, 0] + part[:, j - 1, 1] (csrc/warp_fit.hip)."""
    if not x.is_cuda:
        raise RuntimeError("warp_wgrad: tensors must be on the GPU (no CPU fallback)")
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] >= length >= 1 and length <= 1 << 30, \
        ("warp_wgrad", x.shape, length)
    B = x.shape[0]
    assert dy.is_cuda and dy.device == x.device and dy.dtype == torch.float32 and dy.is_contiguous() and tuple(dy.shape) == (B, length), \
        ("warp_wgrad", dy.shape, (B, length))
    ds = _warp_delay_stride("warp_wgrad", delay, x, B, length)
    part = torch.empty(B, -(-length // 64), 2, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dmx_warp_wgrad(_p(dy), _p(x), x.stride(0), _p(delay), ds, _p(part), min(B, 65536), length, _stream()), "warp_wgrad")
    return part


def warp_update(part, coarse, m, v, fine, length, knot_stride, k, lr, beta1, beta2, eps, max_delay, mean):
    """One Adam step on the coarse knots from the pairs of `warp_wgrad`, minus the mean of the stepped knots when `mean`, the clamp to
    +-max_delay, and the expansion into the fine curve; coarse, m, v (B, P + 1) and fine (B, H + 1) are updated IN PLACE, P = ceil(H /
    knot_stride), k the 1-based count of updates since the last reset.  A clip whose gradient or step is not finite keeps its state."""
    if not part.is_cuda:
        raise RuntimeError("warp_update: tensors must be on the GPU (no CPU fallback)")
    assert 1 <= length <= 1 << 30 and 1 <= knot_stride <= 64, ("warp_update", length, knot_stride)
    H = -(-length // 64)
    P = -(-H // knot_stride)
    assert part.dtype == torch.float32 and part.dim() == 3 and part.is_contiguous() and part.shape[0] >= 1 and \
        tuple(part.shape[1:]) == (H, 2), ("warp_update", tuple(part.shape), (H, 2))
    B = part.shape[0]
    for t, n in ((coarse, P + 1), (m, P + 1), (v, P + 1), (fine, H + 1)):
        assert t.is_cuda and t.device == part.device and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, n), \
            ("warp_update", tuple(t.shape), (B, n))
    _lib.check(_lib.lib().dmx_warp_update(_p(part), _p(coarse), _p(m), _p(v), _p(fine), B, length, int(knot_stride), int(k), float(lr),
                                          float(beta1), float(beta2), float(eps), float(max_delay), 1 if mean else 0, _stream()), "warp_update")


def _click_mask_stride(who, mask, like, B, L):
    assert mask.is_cuda and mask.device == like.device and mask.dtype == torch.float32 and mask.is_contiguous() and \
        tuple(mask.shape) in ((L,), (B, L)), (who, tuple(mask.shape), "expected", (L,), "or", (B, L))
    return 0 if mask.dim() == 1 else L


def click_detect(y, L, threshold, sigma_floor):
    """y (B, >= L) with any row stride -> (a (B, F, 16), e (B, L), sigma (B, F), flags (B, L) uint8, r (B, F, 17)), F = ceil(L / 1024): the
    autoregressive click detector of csrc/declick.hip, frame by frame -- autocorrelation, predictor, residual, robust scale, flags."""
    if not y.is_cuda:
        raise RuntimeError("click_detect: tensors must be on the GPU (no CPU fallback)")
    assert y.dtype == torch.float32 and y.dim() == 2 and y.stride(1) == 1 and y.shape[1] >= L >= 1 and L <= 1 << 30, ("click_detect", y.shape, L)
    B, F = y.shape[0], -(-L // 1024)
    f32 = dict(dtype=torch.float32, device=y.device)
    a, e, sigma, r = torch.empty(B, F, 16, **f32), torch.empty(B, L, **f32), torch.empty(B, F, **f32), torch.empty(B, F, 17, **f32)
    flags = torch.empty(B, L, dtype=torch.uint8, device=y.device)
    _lib.check(_lib.lib().dmx_click_detect(_p(y), y.stride(0), _p(a), _p(e), _p(sigma), _p(flags), _p(r), min(B, 65536), L, threshold, sigma_floor,
                                           _stream()), "click_detect")
    return a, e, sigma, flags, r


def click_mask(flags, guard):
    """flags (B, L) contiguous uint8 -> (mask (B, L) fp32: 0 within `guard` samples of a flag, else 1; masked (B) int32: the zeros per clip)."""
    if not flags.is_cuda:
        raise RuntimeError("click_mask: tensors must be on the GPU (no CPU fallback)")
    assert flags.dtype == torch.uint8 and flags.dim() == 2 and flags.is_contiguous() and 1 <= flags.shape[1] <= 1 << 30, ("click_mask", flags.shape)
    B, L = flags.shape
    mask = torch.empty(B, L, dtype=torch.float32, device=flags.device)
    masked = torch.empty(B, dtype=torch.int32, device=flags.device)
    _lib.check(_lib.lib().dmx_click_mask(_p(flags), _p(mask), _p(masked), min(B, 65536), L, max(min(int(guard), 1 << 20), -1), _stream()),
               "click_mask")
    return mask, masked


def mask_rows(x, mask, L, Ly):
    """x (B, >= L) with any row stride, mask (L) for every clip or (B, L) contiguous -> (B, Ly): x[:, :L] * mask, zeros on [L, Ly)."""
    if not x.is_cuda:
        raise RuntimeError("mask_rows: tensors must be on the GPU (no CPU fallback)")
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] >= L >= 1 and L <= Ly <= 1 << 30, \
        ("mask_rows", x.shape, L, Ly)
    B = x.shape[0]
    ms = _click_mask_stride("mask_rows", mask, x, B, L)
    y = torch.empty(B, Ly, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dmx_mask_rows(_p(x), x.stride(0), _p(mask), ms, _p(y), min(B, 65536), L, Ly, _stream()), "mask_rows")
    return y


def declick_blend(x, y, mask, L, fade):
    """x (restored) and y (measurement) (B, >= L) with any row strides, mask (L) or (B, L) -> (B, L): y away from the mask's zeros, x on them,
    a linear cross-fade over `fade` samples on each side."""
    if not x.is_cuda:
        raise RuntimeError("declick_blend: tensors must be on the GPU (no CPU fallback)")
    for t in (x, y):
        assert t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[1] >= L >= 1 and L <= 1 << 30, ("declick_blend", t.shape, L)
    assert y.shape[0] == x.shape[0] and y.device == x.device, (x.shape, y.shape)
    B = x.shape[0]
    ms = _click_mask_stride("declick_blend", mask, x, B, L)
    out = torch.empty(B, L, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dmx_declick_blend(_p(x), x.stride(0), _p(y), y.stride(0), _p(mask), ms, _p(out), min(B, 65536), L,
                                            max(min(int(fade), 1 << 20), -1), _stream()), "declick_blend")
    return out


def tf_gain(audio, x, gain_t, L, Lfull, *, out=None):
    """x (B, >= L) with any row stride, gain_t (frames, 513) shared or (B, frames, 513), frames = ceil(L / 256) + 3 -> (B, Lfull): the
    time-frequency gain A(x[:, :L]) (csrc/tf_gain.hip), +0 past L.  A is symmetric: the same call is the transpose.
    out: caller-owned (B, >= Lfull) fp32 with any row stride; only out[:, :Lfull] is written."""
    _rows("tf_gain", x, L)
    B, T = x.shape[0], _lib.lib().dmx_audio_tf_frames(L)
    assert Lfull >= L, (L, Lfull)
    assert gain_t.is_cuda and gain_t.dtype == torch.float32 and gain_t.is_contiguous() and gain_t.device == x.device and \
        tuple(gain_t.shape) in ((T, 513), (B, T, 513)), ("tf_gain", tuple(gain_t.shape), (B, T, 513))
    if out is None:
        out = torch.empty(B, Lfull, dtype=torch.float32, device=x.device)
    else:
        _rows("tf_gain", out, Lfull)
        assert out.shape[0] == B and out.device == x.device, (out.shape, B)
    _lib.check(_lib.lib().dmx_audio_tf_gain(audio, _p(x), x.stride(0), _p(gain_t), T * 513 if gain_t.dim() == 3 else 0, _p(out), out.stride(0),
                                            B, L, Lfull, _stream()), "tf_gain")
    return out


def _mdct_step(who, x, step_t, L, Lfull):
    _rows(who, x, L)
    B, T = x.shape[0], _lib.lib().dmx_mdct_frames(L)
    assert Lfull >= L, (L, Lfull)
    assert step_t.is_cuda and step_t.dtype == torch.float32 and step_t.is_contiguous() and step_t.device == x.device and \
        tuple(step_t.shape) in ((T, 512), (B, T, 512)), (who, tuple(step_t.shape), (B, T, 512))
    return B, T


def _mdct_out(who, out, x, B, Lfull):
    if out is None:
        return torch.empty(B, Lfull, dtype=torch.float32, device=x.device)
    _rows(who, out, Lfull)
    assert out.shape[0] == B and out.device == x.device, (out.shape, B)
    return out


def mdct_quant(audio, x, step_t, L, Lfull, *, passthrough=False, want_codes=False, out=None):
    """x (B, >= L) with any row stride, step_t (frames, 512) shared or (B, frames, 512), frames = ceil(L / 512) + 1 -> (y (B, Lfull), codes):
    the MDCT quantiser Phi^T Q(Phi x[:, :L]) (csrc/mdct_quant.hip), +0 past L; codes (B, frames, 512) int32 with `want_codes`, else None.
    passthrough: the straight-through transpose Phi^T K Phi instead (K = 0 where the step is +inf, else 1), which codes nothing.
    out: caller-owned (B, >= Lfull) fp32 with any row stride; only out[:, :Lfull] is written."""
    B, T = _mdct_step("mdct_quant", x, step_t, L, Lfull)
    assert not (passthrough and want_codes), "mdct_quant: the pass-through form codes nothing (want_codes goes with the quantiser)"
    out = _mdct_out("mdct_quant", out, x, B, Lfull)
    codes = torch.empty(B, T, 512, dtype=torch.int32, device=x.device) if want_codes else None
    _lib.check(_lib.lib().dmx_mdct_quant(audio, _p(x), x.stride(0), _p(step_t), T * 512 if step_t.dim() == 3 else 0, _p(codes), _p(out),
                                         out.stride(0), B, L, Lfull, 1 if passthrough else 0, _stream()), "mdct_quant")
    return out, codes


def mdct_project(audio, x, step_t, codes, L, Lfull, *, out=None):
    """x (B, >= L), step_t as in `mdct_quant`, codes (B, frames, 512) int32 of `mdct_quant` -> (B, Lfull): the coefficients of x clamped into
    the cells [(q - 1/2) D, (q + 1/2) D] of the codes on whole frames (1 <= t <= L // 512 - 1) where 0 < D < inf and q is coded, resynthesised."""
    B, T = _mdct_step("mdct_project", x, step_t, L, Lfull)
    assert codes.is_cuda and codes.device == x.device and codes.dtype == torch.int32 and codes.is_contiguous() and \
        tuple(codes.shape) == (B, T, 512), ("mdct_project", tuple(codes.shape), (B, T, 512))
    out = _mdct_out("mdct_project", out, x, B, Lfull)
    _lib.check(_lib.lib().dmx_mdct_project(audio, _p(x), x.stride(0), _p(step_t), T * 512 if step_t.dim() == 3 else 0, _p(codes), _p(out),
                                           out.stride(0), B, L, Lfull, _stream()), "mdct_project")
    return out


def tf_curve(audio, x, curve, L, Lfull):
    """x (B, >= L) with any row stride, curve (513,) shared or (B, 513) -> (B, Lfull): `tf_gain` with a gain constant in time, every frame
    reading the clip's one row (csrc/tf_gain.hip, frame stride 0), +0 past L.  Symmetric: the same call is the transpose."""
    _rows("tf_curve", x, L)
    B = x.shape[0]
    assert Lfull >= L, (L, Lfull)
    assert curve.is_cuda and curve.dtype == torch.float32 and curve.is_contiguous() and curve.device == x.device and \
        tuple(curve.shape) in ((513,), (B, 513)), ("tf_curve", tuple(curve.shape), (B, 513))
    out = torch.empty(B, Lfull, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dmx_audio_tf_curve(audio, _p(x), x.stride(0), _p(curve), 513 if curve.dim() == 2 else 0, _p(out), Lfull, B, L, Lfull,
                                             _stream()), "tf_curve")
    return out


def tf_wgrad(audio, dy, x, L):
    """The gradient of a loss in the curve as partial sums: dy = dLoss/dy and x, both (B, >= L) with any row stride -> (B, segments, 513);
    row s holds the terms of frames [16 s, 16 s + 16), dg = the sum over s (`eq_update` adds the rows in order)."""
    _rows("tf_wgrad", x, L)
    _rows("tf_wgrad", dy, L)
    B = x.shape[0]
    assert dy.shape[0] == B and dy.device == x.device, (dy.shape, x.shape)
    lib = _lib.lib()
    part = torch.empty(B, lib.dmx_audio_tf_wgrad_segments(L), 513, dtype=torch.float32, device=x.device)
    _lib.check(lib.dmx_audio_tf_wgrad(audio, _p(x), x.stride(0), _p(dy), dy.stride(0), _p(part), B, L, _stream()), "tf_wgrad")
    return part


def eq_update(partials, g, m, v, k, lr, beta1, beta2, eps, peak):
    """One Adam step on the curves from the partial rows of `tf_wgrad`, the clamp at zero, then g <- g / max g per clip when `peak`; g, m,
    v (B, 513) are updated IN PLACE, k is the 1-based count of updates since the last reset.  A clip whose gradient or step is not finite,
    or whose peak would be zero, keeps its state."""
    assert partials.is_cuda and partials.dtype == torch.float32 and partials.dim() == 3 and partials.is_contiguous() and \
        partials.shape[2] == 513, partials.shape
    B, segments, n = partials.shape
    for t in (g, m, v):
        assert _taps("eq_update", t, B) == n and t.device == partials.device, (t.shape, partials.shape)
    _lib.check(_lib.lib().dmx_audio_eq_update(_p(partials), segments, _p(g), _p(m), _p(v), B, int(k), float(lr), float(beta1), float(beta2),
                                              float(eps), 1 if peak else 0, _stream()), "eq_update")


def noise_add(y, noise, sigma):
    """-> y + sigma * noise (new tensor; y and noise contiguous, same number of elements)."""
    assert y.is_contiguous() and noise.is_contiguous() and y.numel() == noise.numel(), (y.shape, noise.shape)
    out = torch.empty_like(y)
    _lib.check(_lib.lib().dmx_noise_add(_p(y), _p(noise), _p(out), y.numel(), sigma, _stream()), "noise_add")
    return out


def track_stitch_fwd(wav, starts, L, R, T):
    """wav (W, >= L) with any row stride -> the (1, T) track: the windows at `starts`, cross-faded with the overlap taper R."""
    W = wav.shape[0]
    if not wav.is_cuda:
        raise RuntimeError("track_stitch_fwd: wav must be (W, >= L) fp32 on the GPU (no CPU fallback)")
    assert wav.dtype == torch.float32 and wav.dim() == 2 and wav.stride(1) == 1 and len(starts) == W and wav.shape[1] >= L, \
        (wav.shape, len(starts), L)
    track = torch.empty(1, T, dtype=torch.float32, device=wav.device)
    arr = (C.c_int * W)(*[int(s) for s in starts])
    _lib.check(_lib.lib().dmx_track_stitch_fwd(_p(wav), wav.stride(0), _p(track), arr, W, L, R, T, _stream()), "track_stitch_fwd")
    return track


def track_stitch_bwd(dtrack, starts, L, R, Lfull):
    """The transpose: dtrack (1, T) contiguous -> (W, Lfull), zeros past L."""
    W = len(starts)
    if not dtrack.is_cuda:
        raise RuntimeError("track_stitch_bwd: dtrack must be a GPU tensor (no CPU fallback)")
    assert dtrack.dtype == torch.float32 and dtrack.is_contiguous() and W >= 1, dtrack.shape
    dwav = torch.empty(W, Lfull, dtype=torch.float32, device=dtrack.device)
    arr = (C.c_int * W)(*[int(s) for s in starts])
    _lib.check(_lib.lib().dmx_track_stitch_bwd(_p(dtrack), _p(dwav), Lfull, arr, W, L, R, dtrack.numel(), Lfull, _stream()),
               "track_stitch_bwd")
    return dwav


def _gains_arg(what, gains, K):
    """gains (None = all ones, else K numbers) -> the host float array the launchers take (NULL for None)."""
    if gains is None:
        return None
    if len(gains) != K:
        raise RuntimeError(f"{what}: {len(gains)} gains for {K} stems")
    return (C.c_float * len(gains))(*[float(g) for g in gains])


def _stem_rows(what, x, rows, L):
    if not x.is_cuda:
        raise RuntimeError(f"{what}: a GPU tensor is required (no CPU fallback)")
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or x.shape[0] != rows or x.shape[1] < L:
        raise RuntimeError(f"{what}: expected ({rows}, >= {L}) fp32 with unit column stride, got {tuple(x.shape)} {x.dtype}")


def stem_mix_fwd(wav, gains, K, G, L):
    """wav (K * G, >= L), rows stem-major, any row stride -> the (G, L) mixtures ((g_0 x_0 + g_1 x_1) + ...); gains None = all ones."""
    _stem_rows("stem_mix_fwd", wav, K * G, L)
    arr = _gains_arg("stem_mix_fwd", gains, K)
    mix = torch.empty(max(G, 0), max(L, 0), dtype=torch.float32, device=wav.device)
    _lib.check(_lib.lib().dmx_stem_mix_fwd(_p(wav), wav.stride(0), _p(mix), arr, K, G, L, _stream()), "stem_mix_fwd")
    return mix


def stem_mix_bwd(dmix, gains, K, Lfull):
    """The transpose: dmix (G, L) contiguous -> (K * G, Lfull), row k * G + w = g_k * dmix[w], zeros past L."""
    if not dmix.is_cuda:
        raise RuntimeError("stem_mix_bwd: dmix must be a GPU tensor (no CPU fallback)")
    if dmix.dtype != torch.float32 or dmix.dim() != 2 or not dmix.is_contiguous():
        raise RuntimeError(f"stem_mix_bwd: dmix must be contiguous (G, L) fp32, got {tuple(dmix.shape)} {dmix.dtype}")
    G, L = dmix.shape
    arr = _gains_arg("stem_mix_bwd", gains, K)
    dwav = torch.empty(max(K, 0) * G, max(Lfull, 0), dtype=torch.float32, device=dmix.device)
    _lib.check(_lib.lib().dmx_stem_mix_bwd(_p(dmix), _p(dwav), Lfull, arr, K, G, L, Lfull, _stream()), "stem_mix_bwd")
    return dwav


def stem_project(x, y, gains, L):
    """x (K, >= L) stems, y (1, L) mixture -> (K, L): x_k + c_k (y - mix(x)), c_k = g_k / sum g^2; afterwards the stems sum to y."""
    K = x.shape[0] if x.dim() == 2 else 0
    _stem_rows("stem_project", x, K, L)
    if not y.is_cuda or y.dtype != torch.float32 or not y.is_contiguous() or y.numel() != L or y.device != x.device:
        raise RuntimeError(f"stem_project: y must be a contiguous (1, {L}) fp32 tensor on x's device, got {tuple(y.shape)}")
    arr = _gains_arg("stem_project", gains, K)
    out = torch.empty(K, L, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dmx_stem_project(_p(x), x.stride(0), _p(y), _p(out), arr, K, L, _stream()), "stem_project")
    return out


def stft_mag_fwd(audio, wav, state, L):
    lib = _lib.lib()
    B = wav.shape[0]
    mag = torch.empty(B, lib.dmx_audio_num_bins(audio), lib.dmx_audio_num_frames(audio, L), dtype=torch.float32, device=wav.device)
    _lib.check(lib.dmx_audio_stft_mag(audio, _p(wav), wav.stride(0), _p(mag), _p(state), B, L, _stream()), "stft_mag")
    return mag


def stft_mag_bwd(audio, dmag, state, L, Lfull, *, dwav=None):
    """dwav: caller-owned (B, >= L) result with any row stride, overwritten up to L; without it -> (B, Lfull) with zeros past L."""
    B = dmag.shape[0]
    if dwav is None:
        dwav = torch.zeros(B, Lfull, dtype=torch.float32, device=dmag.device)
    else:
        _rows("stft_mag_bwd", dwav, L)
    _lib.check(_lib.lib().dmx_audio_stft_mag_bwd(audio, _p(dmag), _p(dwav), dwav.stride(0), _p(state), B, L, 0, _stream()), "stft_mag_bwd")
    return dwav


def melscale_fwd(audio, mag, lo, hi):
    B, _, T = mag.shape
    mel = torch.empty(B, T, 64, dtype=torch.float32, device=mag.device)
    _lib.check(_lib.lib().dmx_audio_melscale(audio, _p(mag), _p(mel), B, T, lo, hi, _stream()), "melscale")
    return mel


# ---- networks (workspaces are caller-owned byte tensors sized by *_workspace_bytes)
def unet_fwd(model, x, t, class_labels, ws, c0=None, c1=None, bias1=None, *, out_channels=None):
    """c0 (B, n0, d0), c1 (B, n1, d1), bias1 (B, n1): the two context streams of the AudioLDM2 U-Net and the additive key bias of the
    second, all three or none.  out_channels: of the U-Net when they differ from x's -> eps (B, out_channels or C, h, w)."""
    if not ((c0 is None) == (c1 is None) == (bias1 is None)):
        raise RuntimeError("unet_fwd: c0, c1 and bias1 go together, all three or none")
    B, Cin, h, w = x.shape
    n0, n1 = (c0.shape[1], c1.shape[1]) if c0 is not None else (0, 0)
    eps = torch.empty(B, Cin if out_channels is None else out_channels, h, w, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().dmx_unet_fwd_ctx(model, _p(x), _p(t), _p(class_labels), _p(c0), n0, _p(c1), n1, _p(bias1), _p(eps), B, h, w,
                                           _p(ws), ws.numel(), _stream()), "unet_fwd")
    return eps


def vae_dec_fwd(model, z, z_scale, keep_state, want_f32, scale_factor, ws):
    """-> (mel 16-bit, mel fp32 or None)."""
    B, _, h, w = z.shape
    s = scale_factor
    mel = torch.empty(B, h * s, w * s, dtype=_lib.act_dtype(), device=z.device)
    mel32 = torch.empty(B, h * s, w * s, dtype=torch.float32, device=z.device) if want_f32 else None
    _lib.check(_lib.lib().dmx_vae_decode_fwd(model, _p(z), z_scale, _p(mel), _p(mel32), B, h, w, int(keep_state), _p(ws), ws.numel(),
                                             _stream()), "vae_decode_fwd")
    return mel, mel32


def vae_dec_bwd(model, dmel, z_scale, latent_channels, scale_factor):
    B, H, W = dmel.shape
    dz = torch.empty(B, latent_channels, H // scale_factor, W // scale_factor, dtype=torch.float32, device=dmel.device)
    _lib.check(_lib.lib().dmx_vae_decode_bwd(model, _p(dmel), z_scale, _p(dz), _stream()), "vae_decode_bwd")
    return dz


def vae_enc_fwd(model, mel, log_floor, latent_channels, scale_factor, ws):
    """mel (B, frames, bins) fp32 -> moments (B, (frames / s) * (bins / s), 2 * latent_channels) fp32, [mean | logvar] per position."""
    B, T, F = mel.shape
    s = scale_factor
    mom = torch.empty(B, (T // s) * (F // s), 2 * latent_channels, dtype=torch.float32, device=mel.device)
    _lib.check(_lib.lib().dmx_vae_encode_fwd(model, _p(mel), log_floor, _p(mom), B, T, F, _p(ws), ws.numel(), _stream()), "vae_encode_fwd")
    return mom


def latent_init(moments, h, w, eps, noise, sqrt_abar, scaling_factor, sqrt_1m_abar, want_x):
    """-> (mean, logvar clamped to [-30, 20], x or None), each (B, L, h, w) fp32; x = sqrt_abar * scaling_factor * (mean + std * eps) +
    sqrt_1m_abar * noise (eps None: the mode, noise None: no noise term) when want_x."""
    B, P, L2 = moments.shape
    assert P == h * w and L2 % 2 == 0, (moments.shape, h, w)
    L = L2 // 2
    mean = torch.empty(B, L, h, w, dtype=torch.float32, device=moments.device)
    logvar = torch.empty_like(mean)
    x = torch.empty_like(mean) if want_x else None
    _lib.check(_lib.lib().dmx_latent_init(_p(moments), _p(mean), _p(logvar), _p(x), _p(eps), _p(noise), B, L, P, sqrt_abar,
                                          scaling_factor, sqrt_1m_abar, _stream()), "latent_init")
    return mean, logvar, x


def grad_normalize_(dwav, target):
    """In place on dwav (B, samples): max |g| -> target per clip; returns the factors that undo it."""
    inv_scale = torch.empty(dwav.shape[0], dtype=torch.float32, device=dwav.device)
    _lib.check(_lib.lib().dmx_grad_normalize(_p(dwav), _p(inv_scale), dwav.shape[0], dwav.shape[1], target, _stream()), "grad_normalize")
    return inv_scale


def hifigan_fwd(model, mel, ws, s0=0, s1=0):
    """[s0, s1): samples of every clip that the caller's loss never looks at: zeros there, the same bits elsewhere (an empty span: the
    plain forward)."""
    B, T, _ = mel.shape
    lib = _lib.lib()
    wav = torch.empty(B, lib.dmx_hifigan_out_len(model, T), dtype=torch.float32, device=mel.device)
    _lib.check(lib.dmx_hifigan_fwd_dead(model, _p(mel), _p(wav), B, T, int(s0), int(s1), _p(ws), ws.numel(), _stream()), "hifigan_fwd")
    return wav


def hifigan_dead_plan(model, stages):
    """What the last hifigan forward skipped -> [skipped, total, lo, hi] per stage, flat (dmx_hifigan_dead_plan)."""
    n = int(stages)
    arr = [(C.c_int * n)() for _ in range(4)]
    if _lib.lib().dmx_hifigan_dead_plan(model, *arr, n) < 0:
        _lib.check(-1, "hifigan_dead_plan")
    return [int(a[s]) for s in range(n) for a in arr]


def hifigan_bwd(model, dwav, frames, model_in_dim):
    dmel = torch.empty(dwav.shape[0], frames, model_in_dim, dtype=_lib.act_dtype(), device=dwav.device)
    _lib.check(_lib.lib().dmx_hifigan_bwd(model, _p(dwav), _p(dmel), _stream()), "hifigan_bwd")
    return dmel


# ---- CLAP HTS-AT tower of the style-guidance operator and the Gram matrix of its token features
def htsat_fwd(model, mel, keep_state, ws):
    lib = _lib.lib()
    B, frames, _ = mel.shape
    tokens, channels = C.c_int(), C.c_int()
    _lib.check(lib.dmx_htsat_feature_dims(model, C.byref(tokens), C.byref(channels)), "htsat dims")
    feat = torch.empty(B, tokens.value, channels.value, dtype=torch.float32, device=mel.device)
    _lib.check(lib.dmx_htsat_fwd(model, _p(mel), B, frames, _p(feat), int(keep_state), _p(ws), ws.numel(), _stream()), "htsat_fwd")
    return feat


def htsat_bwd(model, dfeat, scale, frames, bins):
    dmel = torch.empty(dfeat.shape[0], frames, bins, dtype=torch.float32, device=dfeat.device)
    _lib.check(_lib.lib().dmx_htsat_bwd(model, _p(dfeat), _p(scale), _p(dmel), _stream()), "htsat_bwd")
    return dmel


def gram_fwd(feat):
    B, T, Cc = feat.shape
    g = torch.empty(B, Cc, Cc, dtype=torch.float32, device=feat.device)
    _lib.check(_lib.lib().dmx_gram_fwd(_p(feat), _p(g), B, T, Cc, _stream()), "gram_fwd")
    return g


def gram_bwd(feat, dgram):
    B, T, Cc = feat.shape
    d = torch.empty_like(feat)
    _lib.check(_lib.lib().dmx_gram_bwd(_p(feat), _p(dgram), _p(d), B, T, Cc, _stream()), "gram_bwd")
    return d
