"""Blind operators (extensions; every operator of the reference knows its own parameters): measurement operators that fit parameters of
their own inside the guided loop, in the alternating scheme of blind DPS / BUDDy.  One `guidance` call computes the loss and the gradient
w.r.t. the audio with the current estimate, then takes one Adam step on the estimate from the same cotangent (`BaseOperator.after_cotangent`).

`_FittedOperator` holds what they share: the Adam arguments, the life-cycle of the per-clip state and the rule for when a step updates.
A fitted operator provides
  * the key of its state -- the arguments of `_ready(*key)`, which `apply` calls: (batch, device), with the clip length where the shapes
    depend on it -- and `_allocate(*key)` / `_fill()`, which make the tensors (`_m`, `_v` and the estimate) and write `init` into them,
  * `_update(x, length, dy)`, the two launches of one step (gradient in the parameters, Adam + projection),
  * `pin_kwarg` / `update_kwarg`, the names of `apply`'s keyword that pins the parameters of one call and of its flag that freezes the estimate,
  * `positional_state`, the words of the pipelines' refusal of clip lanes and sharding (the state is indexed by batch position).
The pipelines and the schedulers need no edit for a new one."""
import math
import numpy as np
import torch

from .. import ops
from . import dsp
from .operator import DynamicRangeOperator, MusicDereverberationOperator, _MelOperator


class _FittedOperator(_MelOperator):
    """A mel operator with per-clip parameters of its own, fitted by one Adam step per guided step.

    State: `_ready(*key)` makes it on first use and again when the key changes, then puts it to its start; reset_cache() (every
    `set_timesteps`) and restart() (NaN-retry) put it back to the start as well -- the estimate as `_fill` writes it, zero moments, k = 0 --
    so two identical pipeline calls give the same bits.  k, the count of updates since then, is kept on the host and shared by the clips.
    Step: `after_cotangent` updates unless the call pinned the parameters (`pin_kwarg` given: they are used and never updated) or froze the
    estimate (`update_kwarg` False)."""
    pin_kwarg = update_kwarg = None
    k = 0
    _made = None                                              # the key the state was made for
    _m = _v = None                                            # Adam moments, shaped like the fitted tensor

    @staticmethod
    def _adam_args(lr, betas, adam_eps, unit=""):
        """-> (lr, betas, adam_eps), refused by name.  lr: one rate (-> float), or a dict of rates refused by key (returned as it is; a
        bool is no rate there).  unit: what the refusal adds about the rate's unit."""
        per_key = isinstance(lr, dict)
        for what, v in ([(f"lr[{n!r}] = ", v) for n, v in lr.items()] if per_key else [("lr = ", lr)]):
            if not (isinstance(v, (int, float)) and not (per_key and isinstance(v, bool)) and math.isfinite(v) and v > 0):
                raise ValueError(f"{what}{v!r}: a positive number{unit}")
        if len(betas) != 2 or not all(isinstance(b, (int, float)) and 0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"betas = {betas!r}: two numbers in [0, 1)")
        if not (isinstance(adam_eps, (int, float)) and math.isfinite(adam_eps) and adam_eps >= 0):
            raise ValueError(f"adam_eps = {adam_eps!r}: a non-negative number")
        return lr if per_key else float(lr), (float(betas[0]), float(betas[1])), float(adam_eps)

    # ---- the estimate and its optimiser state
    def _allocate(self, *key):
        """Make the state's tensors for `key`; a mismatched `init` is refused before anything is allocated."""
        raise NotImplementedError

    def _fill(self):
        """Write `init` into the estimate (the moments and k are the base's)."""
        raise NotImplementedError

    def _ready(self, *key):
        if self._made != key:
            self._allocate(*key)
            self._made = key
            self._to_start()

    def _to_start(self):
        if self._made is not None:
            self._fill()
            self._m.zero_()
            self._v.zero_()
        self.k = 0

    def reset_cache(self):
        super().reset_cache()
        self._to_start()

    def restart(self):
        self._to_start()

    # ---- the step
    def _update(self, x, length, dy):
        """estimate_k -> estimate_{k+1} (self.k is already k + 1): the gradient in the parameters of this step's cotangent and one Adam +
        projection step, two launches, no host sync."""
        raise NotImplementedError

    def after_cotangent(self, x, length, dy, **apply_kw):
        if apply_kw.get(self.pin_kwarg) is not None or not apply_kw.get(self.update_kwarg, True):
            return
        self.k += 1
        self._update(x, length, dy)


MAX_BLIND_TAPS = 8192     # csrc/fir_blind.hip: the update is one workgroup per clip


class BlindDereverberationOperator(_FittedOperator):
    """Dereverberation with an UNKNOWN impulse response (extension; the reference's operator always knows the response it drew): every
    clip b has its own estimate h[b] (`ir_estimate`, (B, n) fp32 on the GPU), fitted inside the guided loop in the alternating scheme of
    blind DPS / BUDDy.  One `guidance` call computes the loss and the gradient w.r.t. the audio with the current estimate h_k, then takes
    one Adam step on the taps from the same cotangent dy, g[b, t] = sum_o dy[b, o] x[b, o + t - n // 2], followed by the peak normalisation
    h <- h' / max|h'| of `generate_impulse_response`, which pins the scale ambiguity between h and x.  All of it is HIP: `fir_clip_fwd` /
    `fir_clip_bwd` (one response per clip), `fir_wgrad` and `ir_update` (csrc/fir_blind.hip); a clip whose g or step is not finite keeps its
    estimate and moments, and the pipeline's NaN-retry restarts the trajectory (`restart`).

    forward(data, ir=None) makes the measurement with the TRUE response: `ir` ((n,) or (B, n)), or one draw of
    `generate_impulse_response(ir_length, decay_factor)` per clip on the first call, kept as `true_ir` (B, n).
    init: "impulse" (h[n // 2] = 1: A = identity) or an (n,) / (B, n) tensor, peak-normalised per row.
    reset_cache() (every `set_timesteps`) and restart() (NaN-retry) put the estimate back to `init`, zero the moments and set k = 0, so two
    identical pipeline calls give the same bits.  `guidance(..., update_ir=False)` (through the scheduler: `op_kwargs=dict(update_ir=False)`)
    freezes the estimate; `ir=` pins the response of one call and never updates.

    Norms: the update uses the cotangent of the PER-CLIP loss ||.||_2 that `guidance` returns.  A scheduler with per_clip_norm=False rescales
    dwav afterwards by loss_b / ||loss||; for the taps that would only scale g per clip, which Adam's step ignores up to `adam_eps`.

    The state is indexed by batch position, so the pipelines refuse `lanes > 1` and `shard=True` with this operator; inside a TrackOperator
    the batch is the one track.  k, the count of updates since the last reset, is kept on the host and shared by the clips: a clip whose
    update was refused is at most a restart away from k = 0 again."""
    pin_kwarg, update_kwarg = "ir", "update_ir"
    positional_state = ("BlindDereverberationOperator", "response estimates")

    def __init__(self, ir_length=800, decay_factor=0.85, noiser=None, lr=0.05, betas=(0.9, 0.999), adam_eps=1e-8, init="impulse"):
        n = int(ir_length)
        if n < 1 or n > MAX_BLIND_TAPS:
            raise ValueError(f"ir_length = {ir_length!r}: 1 .. {MAX_BLIND_TAPS} taps (the update kernel holds one clip per workgroup)")
        self.lr, self.betas, self.adam_eps = self._adam_args(lr, betas, adam_eps)
        self.ir_length, self.decay_factor, self.noiser = n, decay_factor, noiser
        if isinstance(init, str):
            if init != "impulse":
                raise ValueError(f"init = {init!r}: 'impulse' or an (n,) / (B, n) tensor")
            start = torch.zeros(1, n)
            start[0, n // 2] = 1.0
        else:
            start = torch.as_tensor(init, dtype=torch.float32).detach().cpu()
            if start.dim() not in (1, 2) or start.shape[-1] != n or start.numel() == 0:
                raise ValueError(f"init has shape {tuple(start.shape)}: ({n},) or (B, {n}) for ir_length = {n}")
            start = start.reshape(-1, n).clone()
            peak = start.abs().amax(dim=1, keepdim=True)
            if not bool(torch.isfinite(start).all()) or not bool((peak > 0).all()):
                raise ValueError("init: finite responses with a non-zero peak")
            start = start / peak
        self._start = start                                   # host, (1, n) for every clip or (B, n)
        self.true_ir = None
        self._h = self._h_rev = None
        self._init_mel(16000, lazy=True)

    generate_impulse_response = MusicDereverberationOperator.generate_impulse_response

    # ---- the estimate and its optimiser state
    def _rows(self, ir, batch, what):
        """(n,) / (1, n) / (batch, n) -> host (batch, n) fp32."""
        ir = torch.as_tensor(ir).detach().to(device="cpu", dtype=torch.float32).reshape(-1, self.ir_length)
        if ir.shape[0] not in (1, batch):
            raise ValueError(f"{what} holds {ir.shape[0]} response(s), the batch has {batch} clip(s)")
        return ir.expand(batch, self.ir_length)

    def _allocate(self, batch, device):
        """The (batch, n) estimate with its reverse and Adam moments on `device`."""
        self._rows(self._start, batch, "init")
        self._h, self._h_rev, self._m, self._v = (torch.empty(batch, self.ir_length, dtype=torch.float32, device=device) for _ in range(4))

    def _fill(self):
        self._h.copy_(self._rows(self._start, self._h.shape[0], "init"))
        self._h_rev.copy_(torch.flip(self._h, dims=[1]))

    @property
    def ir_estimate(self):
        """(B, n) fp32 on the GPU, updated in place by every guided step; None before the first call has fixed the batch."""
        return self._h

    # ---- A
    def forward(self, data, ir=None, **kwargs):
        B = data.shape[0]
        if ir is None:
            if self.true_ir is None or self.true_ir.shape[0] != B:
                self.true_ir = torch.cat([self.generate_impulse_response(self.ir_length, self.decay_factor) for _ in range(B)], dim=0)
            ir = self.true_ir
        else:
            ir = self.true_ir = self._rows(ir, B, "ir").clone()
        return super().forward(data, ir=ir, **kwargs)

    def apply(self, x, length, ir=None, update_ir=True, **kw):
        """ir: the response(s) of this call instead of the estimate ((n,) or (B, n)); the estimate is then neither used nor updated."""
        B = x.shape[0]
        if ir is None:
            self._ready(B, x.device)
            h, h_rev = self._h, self._h_rev
        else:
            h = self._rows(ir, B, "ir").to(x.device).contiguous()
            h_rev = torch.flip(h, dims=[1]).contiguous()

        def adjoint(dy, full):
            return ops.hip.fir_clip_bwd(dy.contiguous(), h, h_rev, int(length), int(full))
        return ops.hip.fir_clip_fwd(x, h, int(length)), adjoint

    def _update(self, x, length, dy):
        part = ops.hip.fir_wgrad(dy.contiguous(), x, int(length), self.ir_length)
        ops.hip.ir_update(part, self._h, self._h_rev, self._m, self._v, self.k, self.lr, self.betas[0], self.betas[1], self.adam_eps)


class BlindEqualizationOperator(_FittedOperator):
    """Equalisation with an UNKNOWN curve (extension): the time-frequency gain of `TimeFrequencyMaskOperator` constant in time, G[k, t] =
    g[k] -- a tape or microphone colouration, a low-pass at an unknown cut-off, a tone control -- with one estimate g[b] per clip
    (`eq_estimate`, (B, 513) fp32 on the GPU) fitted inside the guided loop.

        A_g = (1 / c) P^T W F^-1 diag(g) F W P      n_fft 1024, hop 256, periodic Hann, the clip ZERO outside [0, L), c = 1.5; A_1 = I

    One `guidance` call computes the loss and the gradient w.r.t. the audio with the current estimate g_k, then takes one Adam step on
    the curve from the same cotangent dy: dg[b, k] = (h_k / 1536) sum_t Re(X[k, t] conj(U[k, t])) with X, U the STFTs of x and dy, the
    clamp at zero (a magnitude response is not negative) and, with normalize="peak", g <- g / max g, which pins the scale ambiguity between
    g and x.  All of it is HIP: `tf_curve` (csrc/tf_gain.hip with frame stride 0; A is symmetric, the adjoint is the same op), `tf_wgrad`
    and `eq_update` (csrc/tf_eq.hip).  A clip whose gradient or step is not finite keeps its estimate and moments.

    forward(data, curve=None) makes the measurement with the TRUE curve ((513,) or (B, 513)) and keeps it as `true_curve` (B, 513); with
    neither an argument nor a kept curve it raises a ValueError (`dsp.eq_curve` and `dsp.lowpass_curve` build one).
    init: "flat" (g = 1: A = identity) or a (513,) / (B, 513) tensor, finite and non-negative; with normalize="peak" it needs a positive
    peak and is peak-normalised per row.  reset_cache() (every `set_timesteps`) and restart() (NaN-retry) put the estimate back to `init`,
    zero the moments and set k = 0, so two identical pipeline calls give the same bits.  `guidance(..., update_eq=False)` (through the
    scheduler: `op_kwargs=dict(update_eq=False)`) freezes the estimate; `curve=` pins the curve of one call and never updates.

    The model is a real, non-negative, time-invariant curve, hence zero-phase: the mel loss cannot tell it from a minimum-phase filter of the
    same magnitude.  The state is indexed by batch position, so the pipelines refuse `lanes > 1` and `shard=True`; inside a TrackOperator
    the batch is the one track.  dead_span stays None: the estimate moves.  k, the count of updates since the last reset, is kept on the
    host and shared by the clips."""
    pin_kwarg, update_kwarg = "curve", "update_eq"
    positional_state = ("BlindEqualizationOperator", "curve estimates")

    def __init__(self, sample_rate=16000, noiser=None, lr=0.05, betas=(0.9, 0.999), adam_eps=1e-8, init="flat", normalize="peak"):
        self.lr, self.betas, self.adam_eps = self._adam_args(lr, betas, adam_eps)
        if normalize not in ("peak", "none"):
            raise ValueError(f"normalize = {normalize!r}: 'peak' or 'none'")
        n = dsp.TF_BINS
        self.sample_rate, self.noiser, self.normalize = sample_rate, noiser, normalize
        if isinstance(init, str):
            if init != "flat":
                raise ValueError(f"init = {init!r}: 'flat' or a ({n},) / (B, {n}) tensor")
            start = torch.ones(1, n)
        else:
            start = torch.as_tensor(init, dtype=torch.float32).detach().cpu()
            if start.dim() not in (1, 2) or start.shape[-1] != n or start.numel() == 0:
                raise ValueError(f"init has shape {tuple(start.shape)}: ({n},) or (B, {n})")
            start = start.reshape(-1, n).clone()
            if not bool(torch.isfinite(start).all()) or not bool((start >= 0).all()):
                raise ValueError("init: finite, non-negative curves")
            if normalize == "peak":
                peak = start.amax(dim=1, keepdim=True)
                if not bool((peak > 0).all()):
                    raise ValueError("init: curves with a positive peak (normalize = 'peak')")
                start = start / peak
        self._start = start                                   # host, (1, 513) for every clip or (B, 513)
        self.true_curve = None
        self._g = None
        self._init_mel(sample_rate, lazy=True)

    # ---- the estimate and its optimiser state
    def _rows(self, curve, batch, what):
        """(513,) / (1, 513) / (batch, 513) -> host (batch, 513) fp32."""
        curve = torch.as_tensor(curve).detach().to(device="cpu", dtype=torch.float32)
        if curve.dim() not in (1, 2) or curve.shape[-1] != dsp.TF_BINS or curve.numel() == 0:
            raise ValueError(f"{what} has shape {tuple(curve.shape)}: ({dsp.TF_BINS},) or (B, {dsp.TF_BINS})")
        curve = curve.reshape(-1, dsp.TF_BINS)
        if curve.shape[0] not in (1, batch):
            raise ValueError(f"{what} holds {curve.shape[0]} curve(s), the batch has {batch} clip(s)")
        return curve.expand(batch, dsp.TF_BINS)

    def _allocate(self, batch, device):
        """The (batch, 513) estimate with its Adam moments on `device`."""
        self._rows(self._start, batch, "init")
        self._g, self._m, self._v = (torch.empty(batch, dsp.TF_BINS, dtype=torch.float32, device=device) for _ in range(3))

    def _fill(self):
        self._g.copy_(self._rows(self._start, self._g.shape[0], "init"))

    @property
    def eq_estimate(self):
        """(B, 513) fp32 on the GPU, updated in place by every guided step; None before the first call has fixed the batch."""
        return self._g

    # ---- A
    def forward(self, data, curve=None, **kwargs):
        B = data.shape[0]
        if curve is None:
            if self.true_curve is None:
                raise ValueError("BlindEqualizationOperator.forward needs the true curve of the measurement: curve=(513,) or (B, 513) "
                                 "(dsp.eq_curve / dsp.lowpass_curve build one); none was given and none is kept")
            curve = self._rows(self.true_curve, B, "true_curve")
        else:
            curve = self.true_curve = self._rows(curve, B, "curve").clone()
        return super().forward(data, curve=curve, **kwargs)

    def apply(self, x, length, curve=None, update_eq=True, **kw):
        """curve: the curve(s) of this call instead of the estimate ((513,) or (B, 513)); the estimate is then neither used nor updated."""
        B = x.shape[0]
        if curve is None:
            self._ready(B, x.device)
            g = self._g
        else:
            g = self._rows(curve, B, "curve").to(x.device).contiguous()
        h = self.frontend._h.value

        def adjoint(dy, full):                                # A_g is symmetric: the transpose is A_g, zero-padded to `full`
            return ops.hip.tf_curve(h, dy.contiguous(), g, int(length), int(full))
        return ops.hip.tf_curve(h, x, g, int(length), int(length)), adjoint

    def _update(self, x, length, dy):
        part = ops.hip.tf_wgrad(self.frontend._h.value, dy.contiguous(), x, int(length))
        ops.hip.eq_update(part, self._g, self._m, self._v, self.k, self.lr, self.betas[0], self.betas[1], self.adam_eps,
                          self.normalize == "peak")


class BlindTimeWarpOperator(_FittedOperator):
    """Wow and flutter with an UNKNOWN delay curve (extension): the operator of `TimeWarpOperator` with one curve estimate per clip fitted
    inside the guided loop (csrc/warp_fit.hip).

    The estimate lives on coarse knots c[0 .. P] (`warp_estimate`, (B, P + 1) fp32 on the GPU), one every S = `knot_stride` fine knots, P + 1
    = dsp.warp_coarse_knots(L, S); the fine curve the kernels of section 8.10 read (`delay_estimate`, (B, H + 1)) is its linear
    interpolation, `dsp.warp_expand`.  The coarse grid is the regulariser: one knot per 64 S samples.  One `guidance` call computes the loss
    and the gradient w.r.t. the audio with the current fine curve (`warp_fwd`, `warp_bwd`), then `warp_wgrad` turns the same cotangent into
    the gradient in the knots and `warp_update` takes one Adam step on c, subtracts the mean of the knots (anchor="mean": a constant delay
    is a shift of x, which the prior cannot tell apart), clamps every knot to +-max_delay and expands: two launches, no host sync.  A clip
    whose gradient or step is not finite keeps its state.  max_delay <= min(4096, 8 S) keeps every curve the update writes inside the
    contract of `warp_bwd` (|c| <= M gives fine steps of at most 2 M / S <= 16), so no slope projection is needed.

    lr is in samples per step (Adam moves a knot by about lr per step); the default is a caller's knob, not a tuned value.
    forward(data, delay=None) makes the measurement with the TRUE fine curve ((H + 1,) or (B, H + 1), `dsp.wow_curve` builds one) and keeps
    it as `true_delay`.  init: "zero" or a coarse curve (P + 1,) / (B, P + 1), finite and within +-max_delay, mean-subtracted per row under
    anchor="mean".  The state is made on first use and again when the batch, length or device changes; reset_cache() (every
    `set_timesteps`) and restart() (NaN-retry) put it back, so two identical pipeline calls give the same bits.
    `guidance(..., update_warp=False)` freezes the estimate; `delay=` (fine knots) pins the curve of one call and never updates.

    The curve is piecewise linear on 64 S-sample knots and boxed to +-8 S samples; a constant delay is not identified under
    anchor="mean"; the fit needs band-limited content (the gradient runs through a cubic's derivative of x).  The state is indexed by batch
    position, so the pipelines refuse `lanes > 1` and `shard=True`.  dead_span stays None.  k, the count of updates since the last reset,
    is kept on the host and shared by the clips."""
    pin_kwarg, update_kwarg = "delay", "update_warp"
    positional_state = ("BlindTimeWarpOperator", "delay-curve estimates")

    def __init__(self, sample_rate=16000, noiser=None, knot_stride=16, max_delay=128.0, lr=0.1, betas=(0.9, 0.999), adam_eps=1e-8, init="zero",
                 anchor="mean"):
        if not (math.isfinite(float(sample_rate)) and float(sample_rate) > 0):
            raise ValueError(f"sample_rate = {sample_rate!r}: a positive finite rate")
        if isinstance(knot_stride, bool) or knot_stride not in dsp.WARP_KNOT_STRIDES:
            raise ValueError(f"knot_stride = {knot_stride!r}: a power of two from 1 to 64 (fine knots per coarse knot)")
        box = min(dsp.WARP_MAX_DELAY, 8.0 * knot_stride)
        if not (isinstance(max_delay, (int, float)) and math.isfinite(max_delay) and 0 < max_delay <= box):
            raise ValueError(f"max_delay = {max_delay!r}: positive and at most min(4096, 8 * knot_stride) = {box:g} samples, which keeps every "
                             "fitted curve inside the contract of the transpose (fine steps of at most 16)")
        self.lr, self.betas, self.adam_eps = self._adam_args(lr, betas, adam_eps, " (samples per step)")
        if anchor not in ("mean", "none"):
            raise ValueError(f"anchor = {anchor!r}: 'mean' or 'none'")
        self.sample_rate, self.noiser, self.anchor = sample_rate, noiser, anchor
        self.knot_stride, self.max_delay = int(knot_stride), float(np.float32(max_delay))
        if isinstance(init, str):
            if init != "zero":
                raise ValueError(f"init = {init!r}: 'zero' or a coarse curve (P + 1,) / (B, P + 1)")
            start = None
        else:
            start = torch.as_tensor(init, dtype=torch.float32).detach().cpu()
            if start.dim() not in (1, 2) or start.shape[-1] < 2 or start.numel() == 0:
                raise ValueError(f"init has shape {tuple(start.shape)}: (P + 1,) or (B, P + 1) coarse knots")
            start = start.reshape(-1, start.shape[-1]).clone()
            if not bool(torch.isfinite(start).all()) or float(start.abs().max()) > self.max_delay:
                raise ValueError(f"init: finite knots within +-max_delay = {self.max_delay:g} samples")
            if anchor == "mean":
                start = (start - start.mean(dim=1, keepdim=True)).clamp_(-self.max_delay, self.max_delay)
        self._start = start                                   # host, None (zeros), (1, P + 1) for every clip or (B, P + 1)
        self.true_delay = None
        self._c = self._d = None
        self._init_mel(sample_rate, lazy=True)

    # ---- the estimate and its optimiser state
    def _start_rows(self, batch, length):
        """host (batch, P + 1) fp32: the coarse curve every trajectory starts from"""
        n = dsp.warp_coarse_knots(length, self.knot_stride)
        if self._start is None:
            return torch.zeros(batch, n)
        if self._start.shape[1] != n or self._start.shape[0] not in (1, batch):
            raise ValueError(f"init holds {self._start.shape[0]} coarse curve(s) of {self._start.shape[1]} knots; a batch of {batch} clip(s) of "
                             f"{length} samples needs (1 or {batch}) x warp_coarse_knots({length}, {self.knot_stride}) = {n}")
        return self._start.expand(batch, n)

    def _allocate(self, batch, length, device):
        """The coarse estimate with its Adam moments and the fine curve on `device`."""
        self._start_rows(batch, length)
        n = dsp.warp_coarse_knots(length, self.knot_stride)
        self._c, self._m, self._v = (torch.empty(batch, n, dtype=torch.float32, device=device) for _ in range(3))
        self._d = torch.empty(batch, dsp.warp_knots(length), dtype=torch.float32, device=device)

    def _fill(self):
        batch, length, _ = self._made
        start = self._start_rows(batch, length)
        self._c.copy_(start)
        self._d.copy_(torch.from_numpy(dsp.warp_expand(start.numpy(), length, self.knot_stride)))

    @property
    def warp_estimate(self):
        """(B, P + 1) fp32 coarse knots on the GPU, updated in place by every guided step; None before the first call."""
        return self._c

    @property
    def delay_estimate(self):
        """(B, H + 1) fp32 fine knots on the GPU: `dsp.warp_expand` of `warp_estimate`, what `warp_fwd` / `warp_bwd` read."""
        return self._d

    # ---- A
    def _fine_rows(self, delay, batch, length, what):
        """(H + 1,) / (1, H + 1) / (batch, H + 1) fine knots -> host (batch, H + 1) fp32, the contract checked by name"""
        d = torch.as_tensor(delay).detach().to(device="cpu", dtype=torch.float32).contiguous()
        dsp.check_warp_curve(d.numpy(), what)
        K = dsp.warp_knots(length)
        d = d.reshape(-1, d.shape[-1])
        if d.shape[1] != K or d.shape[0] not in (1, batch):
            raise ValueError(f"{what} has shape {tuple(d.shape)}: a batch of {batch} clip(s) of {length} samples needs (warp_knots({length}),) = "
                             f"({K},) or ({batch}, {K})")
        return d.expand(batch, K)

    def forward(self, data, delay=None, **kwargs):
        B, L = data.shape[0], data.shape[-1]
        if delay is None:
            if self.true_delay is None:
                raise ValueError("BlindTimeWarpOperator.forward needs the true delay curve of the measurement: delay=(warp_knots(length),) or "
                                 "(B, warp_knots(length)) fine knots (dsp.wow_curve builds one); none was given and none is kept")
            delay = self._fine_rows(self.true_delay, B, L, "true_delay")
        else:
            delay = self.true_delay = self._fine_rows(delay, B, L, "delay").clone()
        return super().forward(data, delay=delay, **kwargs)

    def apply(self, x, length, delay=None, update_warp=True, **kw):
        """delay: the fine curve(s) of this call instead of the estimate; the estimate is then neither used nor updated."""
        B = x.shape[0]
        if delay is None:
            self._ready(B, int(length), x.device)
            d = self._d
        else:
            d = self._fine_rows(delay, B, int(length), "delay").to(x.device).contiguous()

        def adjoint(dy, full):
            return ops.hip.warp_bwd(dy.contiguous(), d, int(length), int(full))
        return ops.hip.warp_fwd(x, d, int(length)), adjoint

    def _update(self, x, length, dy):
        part = ops.hip.warp_wgrad(dy.contiguous(), x, self._d, int(length))
        ops.hip.warp_update(part, self._c, self._m, self._v, self._d, int(length), self.knot_stride, self.k, self.lr, self.betas[0],
                            self.betas[1], self.adam_eps, self.max_delay, self.anchor == "mean")


class BlindDynamicRangeOperator(_FittedOperator):
    """De-compression with UNKNOWN compressor settings (extension): the operator of `DynamicRangeOperator` with one parameter estimate per
    clip fitted inside the guided loop (csrc/drc_fit.hip).

    Per clip the fitted vector is phi = (T, k, m, ln aA, ln aR): threshold in dB, slope k = 1 - 1 / ratio, make-up in dB and the logarithms
    of the attack and release coefficients of `dsp.drc_coeffs`; the knee width `knee_db` is given and shared.  The kernels read the table
    row theta[b] = (T, k, m, aA, aR, 1 - aA, 1 - aR, k / (2 W)) on the device (`drc_fwd_p`, `drc_bwd_p`: the three launches per direction of
    the fixed operator).  One `guidance` call computes the loss and the gradient w.r.t. the audio with the current estimate, then
    `drc_pgrad` turns what the backward follower left into the gradient in phi and `drc_update` takes one Adam step per parameter, clamps it
    to its box and rewrites the row: two launches, no host sync.  A clip whose gradient or step is not finite keeps its state.

    fit names the parameters that move: "threshold", "ratio", "makeup", "attack", "release"; the others stay at `init` (their lr is 0: value,
    moments and table entries keep their bits).  lr is per parameter, in the parameter's own unit per step -- dB for threshold and makeup,
    slope units for the ratio's k, natural-log units of the coefficient for attack and release; Adam moves a parameter by about lr per
    step.  The defaults are callers' knobs, not tuned values.  The boxes: threshold_range and makeup_range in dB, time_range_ms for both
    time constants, k in [0, 1].
    forward(data, params=dict(threshold_db, ratio, attack_ms, release_ms, makeup_db)) makes the measurement with the TRUE parameters through
    the fixed route (`drc_fwd`) and keeps them as `true_params`.  The state is made on first use and again when the batch or the device
    changes; reset_cache() (every `set_timesteps`) and restart() (NaN-retry) put it back, so two identical pipeline calls give the same
    bits.  `guidance(..., update_drc=False)` freezes the estimate; `params=` pins the parameters of one call and never updates.

    The knee width is not fitted; the sidechain runs at block rate; threshold and make-up trade off against each other on material that
    never leaves the compressed region.  The state is indexed by batch position, so the pipelines refuse `lanes > 1` and `shard=True`.
    dead_span stays None.  k, the count of updates since the last reset, is kept on the host and shared by the clips."""
    pin_kwarg, update_kwarg = "params", "update_drc"
    positional_state = ("BlindDynamicRangeOperator", "parameter estimates")

    NAMES = ("threshold", "ratio", "makeup", "attack", "release")          # the order of phi
    LR_KEYS = ("threshold", "slope", "makeup", "attack", "release")
    INIT = dict(threshold_db=-12.0, ratio=2.0, attack_ms=5.0, release_ms=100.0, makeup_db=0.0)
    LR = dict(threshold=0.25, slope=0.01, makeup=0.1, attack=0.02, release=0.02)

    def __init__(self, sample_rate=16000, knee_db=6.0, noiser=None, fit=("threshold", "ratio", "makeup"), init=None, lr=None,
                 betas=(0.9, 0.999), adam_eps=1e-8, threshold_range=(-60.0, 0.0), makeup_range=(-24.0, 24.0), time_range_ms=(0.5, 2000.0)):
        if not (math.isfinite(float(sample_rate)) and float(sample_rate) > 0):
            raise ValueError(f"sample_rate = {sample_rate!r}: a positive finite rate")
        knee = float(knee_db)
        if not (math.isfinite(knee) and 0.0 <= knee <= 200.0):
            raise ValueError(f"knee_db = {knee_db!r}: a finite width in [0, 200]")
        fit = (fit,) if isinstance(fit, str) else tuple(fit)
        if not fit or any(n not in self.NAMES for n in fit) or len(set(fit)) != len(fit):
            raise ValueError(f"fit = {fit!r}: one or more of {self.NAMES}, each once")
        init = dict(self.INIT, **self._known("init", init, self.INIT))
        lr = dict(self.LR, **self._known("lr", lr, self.LR))
        lr, self.betas, self.adam_eps = self._adam_args(lr, betas, adam_eps, " (the parameter's own unit per step)")

        def span(name, r, lo, hi):
            if len(r) != 2 or not all(isinstance(v, (int, float)) and math.isfinite(v) for v in r) or not lo <= r[0] <= r[1] <= hi:
                raise ValueError(f"{name} = {r!r}: (low, high) with {lo} <= low <= high <= {hi}")
            return float(r[0]), float(r[1])
        t_lo, t_hi = span("threshold_range", threshold_range, -200.0, 200.0)
        m_lo, m_hi = span("makeup_range", makeup_range, -200.0, 200.0)
        if len(time_range_ms) != 2 or not all(isinstance(v, (int, float)) and math.isfinite(v) and v > 0 for v in time_range_ms) or \
                time_range_ms[0] > time_range_ms[1]:
            raise ValueError(f"time_range_ms = {time_range_ms!r}: (shortest, longest) positive times in milliseconds")
        a_hi, a_lo = dsp.drc_coeffs(sample_rate, time_range_ms[0], time_range_ms[1])          # the short time has the large coefficient
        ln_lo, ln_hi = math.log(float(a_lo)), math.log(float(a_hi))
        self.sample_rate, self.noiser = sample_rate, noiser
        self.knee_db = float(np.float32(knee))
        self.fit = fit
        self.lr = tuple(float(lr[key]) if name in fit else 0.0 for name, key in zip(self.NAMES, self.LR_KEYS))
        self.box_lo, self.box_hi = (t_lo, 0.0, m_lo, ln_lo, ln_lo), (t_hi, 1.0, m_hi, ln_hi, ln_hi)
        self.init = init
        self._start = self._phi_of(init, "init")                 # (5,) float64: inside the boxes, refused by name otherwise
        for name, v, lo, hi in zip(self.NAMES, self._start, self.box_lo, self.box_hi):
            if not lo - 1e-6 * max(1.0, abs(lo)) <= v <= hi + 1e-6 * max(1.0, abs(hi)):
                raise ValueError(f"init: the {name} parameter starts outside its range (threshold_range, makeup_range, time_range_ms, "
                                 "ratio >= 1)")
        self.true_params = None
        self._phi = self._theta = None
        self._kept = None
        self._init_mel(sample_rate, lazy=True)

    @staticmethod
    def _known(what, given, known):
        given = {} if given is None else dict(given)
        for key in given:
            if key not in known:
                raise ValueError(f"{what}[{key!r}]: unknown key; the keys are {tuple(known)}")
        return given

    def _fixed(self, p, what):
        """dict(threshold_db, ratio, attack_ms, release_ms, makeup_db) -> the six fp32 parameters of `drc_fwd`, refused by name"""
        p = self._known(what, p, self.INIT)
        if set(p) != set(self.INIT):
            raise ValueError(f"{what} needs all of {tuple(self.INIT)}; got {tuple(p)}")
        try:
            return DynamicRangeOperator(sample_rate=self.sample_rate, knee_db=self.knee_db, **p).params
        except ValueError as e:
            raise ValueError(f"{what}: {e}") from None

    def _phi_of(self, p, what):
        T, k, _, aA, aR, mk = self._fixed(p, what)
        return np.array([T, k, mk, math.log(aA), math.log(aR)], dtype=np.float64)

    # ---- the estimate and its optimiser state
    def _allocate(self, batch, device):
        """The table with phi and its Adam moments on `device`; `init` was checked at construction and serves any batch."""
        self._phi, self._m, self._v = (torch.empty(batch, 5, dtype=torch.float32, device=device) for _ in range(3))
        self._theta = torch.empty(batch, 8, dtype=torch.float32, device=device)

    def _fill(self):
        B = self._phi.shape[0]
        T, k, mk, lnA, lnR = self._start
        aA, aR = dsp.drc_coeffs(self.sample_rate, self.init["attack_ms"], self.init["release_ms"])
        self._phi.copy_(torch.from_numpy(np.broadcast_to(self._start.astype(np.float32), (B, 5)).copy()))
        self._theta.copy_(torch.from_numpy(dsp.drc_table(T, k, aA, aR, mk, self.knee_db, B)))

    def _to_start(self):
        super()._to_start()
        self._kept = None

    @property
    def drc_estimate(self):
        """(B, 5) float64 on the host in user units: threshold_db, ratio, makeup_db, attack_ms, release_ms; None before the first call."""
        if self._phi is None:
            return None
        phi = self._phi.detach().cpu().numpy().astype(np.float64)
        with np.errstate(divide="ignore"):
            ratio = 1.0 / (1.0 - phi[:, 1])
        return np.stack([phi[:, 0], ratio, phi[:, 2], dsp.drc_time_ms(np.exp(phi[:, 3]), self.sample_rate),
                         dsp.drc_time_ms(np.exp(phi[:, 4]), self.sample_rate)], axis=1)

    @property
    def phi_estimate(self):
        """(B, 5) fp32 on the GPU: T, k, makeup, ln aA, ln aR, updated in place by every guided step; None before the first call."""
        return self._phi

    @property
    def table_estimate(self):
        """(B, 8) fp32 on the GPU: the rows `drc_fwd_p` / `drc_bwd_p` read."""
        return self._theta

    # ---- A
    def forward(self, data, params=None, **kwargs):
        if params is None:
            if self.true_params is None:
                raise ValueError("BlindDynamicRangeOperator.forward needs the true parameters of the measurement: params=dict(threshold_db, "
                                 "ratio, attack_ms, release_ms, makeup_db); none was given and none is kept")
            params = self.true_params
        else:
            self._fixed(params, "params")                        # refused by name before it is kept
            params = self.true_params = dict(params)
        return super().forward(data, params=params, **kwargs)

    def apply(self, x, length, params=None, update_drc=True, **kw):
        """params: the parameters of this call instead of the estimate, through the fixed route; the estimate is then neither used nor
        updated."""
        if params is not None:
            fixed = self._fixed(params, "params")
            y, state, tape = ops.hip.drc_fwd(x, int(length), *fixed)

            def adjoint(dy, full):
                return ops.hip.drc_bwd(dy, x, state, tape, int(full), *fixed)
            return y, adjoint
        self._ready(x.shape[0], x.device)
        theta, W = self._theta, self.knee_db
        y, state, tape = ops.hip.drc_fwd_p(x, int(length), theta, W)

        def adjoint(dy, full):
            dx, work, bq0 = ops.hip.drc_bwd_p(dy, x, state, tape, theta, int(full), W)
            self._kept = (state, tape, work, bq0)                # what `_update` turns into the parameter gradient
            return dx
        return y, adjoint

    def after_cotangent(self, x, length, dy, **apply_kw):
        """What `adjoint` kept serves one step: it is dropped on every call, whether or not this one updates."""
        try:
            if self._kept is not None:
                super().after_cotangent(x, length, dy, **apply_kw)
        finally:
            self._kept = None

    def _update(self, x, length, dy):
        state, tape, work, bq0 = self._kept
        part = ops.hip.drc_pgrad(state, tape, work, bq0, self._theta, int(length), self.knee_db)
        ops.hip.drc_update(part, self._phi, self._m, self._v, self._theta, int(length), self.k, list(self.lr), self.betas[0], self.betas[1],
                           self.adam_eps, self.knee_db, list(self.box_lo), list(self.box_hi))
