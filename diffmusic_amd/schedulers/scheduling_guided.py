"""The five in-scope schedulers behind the reference's Scheduler protocol:
same constructor keys (configs/model/*.yaml `scheduler:`), `set_timesteps`, `timesteps`,
`scale_model_input`, `init_noise_sigma`, `order`, `config`, and `step(...)` with the reference's
signature (diffmusic/schedulers/scheduling_dps.py:137-156 and siblings).

Host side = DDIM tables and per-step scalars (fp32, computed once; no device sync per step).
Device side = HIP: x0 prediction, VAE decode, HiFi-GAN, measurement operator, mel, L2 loss, the
hand-written backward sweep and the fused update kernel (csrc/sched.hip).  There is no autograd and
no CPU fallback."""
from types import SimpleNamespace
import numpy as np
import torch

from .. import ops
from ..torch_utils import randn_tensor, randn_philox
from ..profiling import stage
from ..inverse_problem.noise import step_sigma
from .utils import InverseProblemSchedulerOutput

_MODE = dict(ddim=0, dps=1, mpgd=2, dsg=3, diffmusic=4)
_PTYPE = dict(epsilon=0, sample=1, v_prediction=2)          # include/diffmusic_hip.h dmx_sched_pred_x0_ex


def rescale_zero_terminal_snr(betas):
    """diffusers `rescale_zero_terminal_snr` (Lin et al. 2023, Algorithm 1): shift / scale sqrt(alpha_bar) so that the last timestep has zero SNR."""
    alphas_bar_sqrt = torch.cumprod(1.0 - betas, dim=0).sqrt()
    a0, aT = alphas_bar_sqrt[0].clone(), alphas_bar_sqrt[-1].clone()
    alphas_bar_sqrt = (alphas_bar_sqrt - aT) * (a0 / (a0 - aT))
    alphas_bar = alphas_bar_sqrt ** 2
    alphas = torch.cat([alphas_bar[0:1], alphas_bar[1:] / alphas_bar[:-1]])
    return 1.0 - alphas


class GuidedDDIMScheduler:
    """Common base: diffusers-0.31.0-compatible DDIM tables + the HIP guided step."""
    order = 1
    init_noise_sigma = 1.0
    mode = "ddim"
    default_eta = 0.0
    default_rate = 0.0
    passes_eta_to_parent = False      # DPS/MPGD: parent DDIM step consumes one randn draw when eta > 0

    def __init__(self, operator=None, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, clip_sample=True, set_alpha_to_one=True, steps_offset=0, prediction_type="epsilon",
                 thresholding=False, dynamic_thresholding_ratio=0.995, clip_sample_range=1.0, sample_max_value=1.0,
                 timestep_spacing="leading", rescale_betas_zero_snr=False, grad_target=64.0, per_clip_norm=True, device_noise=False,
                 *args, **kwargs):
        if prediction_type not in _PTYPE:
            raise ValueError(f"prediction_type given as {prediction_type} must be one of `epsilon`, `sample`, or `v_prediction`")
        if thresholding:
            # (dynamic thresholding rescales x0 by a per-sample quantile of |x0| -- Imagen's trick for pixel-space models; no config of the
            #  reference's latent pipelines selects it: configs/model/*.yaml)
            raise NotImplementedError("thresholding=True (dynamic thresholding of x0) is not built")
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, trained_betas=trained_betas, clip_sample=clip_sample,
                                      set_alpha_to_one=set_alpha_to_one, steps_offset=steps_offset,
                                      prediction_type=prediction_type, thresholding=thresholding,
                                      timestep_spacing=timestep_spacing, rescale_betas_zero_snr=rescale_betas_zero_snr,
                                      clip_sample_range=clip_sample_range)
        self._ptype = _PTYPE[prediction_type]
        self._clip_r = float(clip_sample_range) if clip_sample else 0.0
        if trained_betas is not None:
            betas = torch.tensor(trained_betas, dtype=torch.float32)
        elif beta_schedule == "linear":
            betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        else:
            raise NotImplementedError(f"{beta_schedule} is not implemented")
        if rescale_betas_zero_snr:
            betas = rescale_zero_terminal_snr(betas)
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)            # fp32, host
        if rescale_betas_zero_snr:
            self.alphas_cumprod[-1] = 2 ** -24                             # diffusers: "close to 0 without being 0 so first sigma is not inf"
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self._ac = self.alphas_cumprod.numpy()
        self.operator = operator
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self.grad_target = grad_target
        # True (default): every clip of a batch is guided by its own loss / gradient norms, i.e. a batch equals B independent
        # B = 1 runs (the only case the reference ever ran).  False: the reference's literal whole-tensor norms
        # (torch.linalg.norm over the batch tensor, scheduling_dps.py:205-206; DSG / DiffMusic norms likewise).
        self.per_clip_norm = per_clip_norm
        self.last_grad = None
        self.debug_keep_grad = False
        # False (default): per-step noise comes from `randn_tensor` (host generators, uploaded), bit-identical to the reference's
        # stream.  True: drawn on the device by the Philox kernel (csrc/rng.hip), keyed per clip by the generators' initial seeds
        # -- a different (but equally per-clip, GPU-count-independent) stream, without the host draw and the H2D copy.
        self.device_noise = device_noise
        self._noise_offset = 0

    # ---- protocol pieces the pipelines touch
    def scale_model_input(self, sample, timestep=None):
        return sample

    def set_timesteps(self, num_inference_steps, device=None):
        n_train = self.config.num_train_timesteps
        if num_inference_steps > n_train:
            raise ValueError("num_inference_steps > num_train_timesteps")
        self.num_inference_steps = num_inference_steps
        sp = self.config.timestep_spacing
        if sp == "leading":
            ratio = n_train // num_inference_steps
            ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.config.steps_offset
        elif sp == "trailing":
            ts = np.round(np.arange(n_train, 0, -n_train / num_inference_steps)).astype(np.int64) - 1
        elif sp == "linspace":
            ts = np.linspace(0, n_train - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        else:
            raise ValueError(f"{sp} is not supported")
        self._timesteps_host = [int(t) for t in ts]
        self._noise_offset = 0
        if self.operator is not None and hasattr(self.operator, "reset_cache"):
            self.operator.reset_cache()           # a new trajectory: forget the cached transform(measurement)
        self.timesteps = torch.from_numpy(ts).to(device) if device is not None else torch.from_numpy(ts)

    # ---- warm start (init audio + strength): the trajectory begins at an intermediate timestep of the list set_timesteps(N) made
    def timesteps_for_strength(self, strength):
        """diffusers' img2img rule: the last `min(int(N * strength), N)` timesteps of the current list.  `num_inference_steps` stays N, so
        the step width of `_scalars` and the position of a timestep in the full list (measurement-noise key) are those of a cold run."""
        n = self.num_inference_steps
        if n is None:
            raise ValueError("call set_timesteps(num_inference_steps) before timesteps_for_strength")
        if not 0.0 <= float(strength) <= 1.0:
            raise ValueError(f"strength = {strength!r}: a number in [0, 1]")
        n_run = min(int(n * float(strength)), n)
        if n_run == 0:
            raise ValueError(f"strength = {strength!r} leaves no step of num_inference_steps = {n} to run (int(N * strength) == 0)")
        return list(self._timesteps_host[n - n_run:])

    def add_noise_scalars(self, timestep):
        """(sqrt(abar_t), sqrt(1 - abar_t)) as host floats from the fp32 table."""
        a = float(self._ac[int(timestep)])
        return a ** 0.5, (1.0 - a) ** 0.5

    def add_noise(self, original_samples, noise, timestep):
        """x_t = sqrt(abar_t) x0 + sqrt(1 - abar_t) noise (diffusers `add_noise`, one host timestep for the batch); the sum is the HIP
        `noise_add` launch."""
        if not original_samples.is_cuda:
            raise RuntimeError("diffmusic_amd schedulers run on the GPU only (no CPU fallback)")
        sa, s1 = self.add_noise_scalars(timestep)
        x0 = (original_samples.detach().to(torch.float32) * sa).contiguous()
        z = noise.detach().to(device=x0.device, dtype=torch.float32).contiguous()
        return ops.hip.noise_add(x0, z, float(s1)).to(original_samples.dtype)

    def _get_variance(self, timestep, prev_timestep):
        a_t = float(self._ac[timestep])
        a_p = float(self._ac[prev_timestep]) if prev_timestep >= 0 else float(self.final_alpha_cumprod)
        return (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)

    def _scalars(self, timestep, eta):
        t = int(timestep)                       # a device tensor here costs one sync; the pipeline passes host ints
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = float(self._ac[t])
        a_p = float(self._ac[prev_t]) if prev_t >= 0 else float(self.final_alpha_cumprod)
        sigma = eta * self._get_variance(t, prev_t) ** 0.5
        return t, a_t, a_p, sigma

    # ---- HIP guidance sweep: x0 -> vae -> vocoder -> A -> loss ; and back
    def _op_kwargs(self, op_kwargs, timestep, generator):
        """Keywords of `operator.guidance` for this step.  An operator whose noiser adds Gaussian noise inside the step (noise.py
        `additive_sigma > 0`) also gets the step index -- the position of `timestep` in this trajectory's list, never a call counter -- and
        the generator(s), which key the per-clip measurement-noise stream; `noise=` in op_kwargs (teacher forcing) replaces the draw."""
        if step_sigma(getattr(self.operator, "noiser", None)) <= 0 or "noise" in (op_kwargs or {}):
            return op_kwargs
        ts = getattr(self, "_timesteps_host", None) or []
        return dict(op_kwargs or {}, step=ts.index(timestep) if timestep in ts else None, generator=generator)

    def _guidance(self, x0, measurement, vae, vocoder, length, supervised_space, op_kwargs=None):
        zs = 1.0 / vae.config.scaling_factor
        with stage("vae_fwd"):
            mel = vae.decode_hip(x0, z_scale=zs, keep_state=True)              # (B, H, W) fp16
        with stage("hifigan_fwd"):
            span = getattr(self.operator, "dead_span", None)                   # samples the loss never sees (an inpainting hole), or None
            dead = span(length) if span is not None else None
            wav = vocoder.forward(mel) if dead is None else vocoder.forward(mel, dead=dead)      # (B, Lfull) fp32
        with stage("operator_mel_loss_fwd_bwd"):
            loss, dwav = self.operator.guidance(wav, length, measurement, supervised_space, **(op_kwargs or {}))
            if not self.per_clip_norm and loss.numel() > 1:
                # whole-batch norm: L = sqrt(sum_b L_b^2), dL/dwav_b = (L_b / L) * dL_b/dwav_b  (device-side, B scalars)
                total = torch.linalg.vector_norm(loss)
                dwav.mul_((loss / total.clamp_min(1e-30))[:, None])
                loss = total.reshape(1)
            inv_scale = ops.hip.grad_normalize_(dwav, float(self.grad_target))           # in place on dwav
        with stage("hifigan_bwd"):
            dmel = vocoder.backward(dwav)
        with stage("vae_bwd"):
            g0 = vae.backward(dmel, z_scale=zs)                                # dLoss/dx0 * (1/inv_scale)
        return loss, g0, inv_scale

    def step(self, model_output, timestep, sample, eta=None, use_clipped_model_output=False, generator=None,
             variance_noise=None, return_dict=True, measurement=None, ip_guidance_rate=None, vae=None, vocoder=None,
             original_waveform_length=0, supervised_space="mel_spectrogram", eps=1e-8, *args, **kwargs):
        eta = self.default_eta if eta is None else eta
        rate = self.default_rate if ip_guidance_rate is None else ip_guidance_rate
        if supervised_space not in ("wav_form", "mel_spectrogram"):
            raise ValueError("supervised_space should be either 'wav_form' or 'mel_spectrogram")
        if variance_noise is not None and generator is not None and eta > 0:
            raise ValueError("Cannot pass both generator and variance_noise. Please make sure that either `generator` or"
                             " `variance_noise` stays `None`.")
        one_sample = getattr(self.operator, "one_sample", None)          # TrackOperator, MixtureOperator: the reason, as a sentence
        if self.per_clip_norm and self.mode != "ddim" and one_sample:
            raise ValueError(f"{one_sample}: construct the scheduler with per_clip_norm=False")
        if not sample.is_cuda:
            raise RuntimeError("diffmusic_amd schedulers run on the GPU only (no CPU fallback)")
        if self._ptype == 1 and self.mode in ("dps", "dsg", "diffmusic"):
            raise RuntimeError("prediction_type='sample': pred_original_sample = model_output does not depend on the sample, so the gradient of "
                               "the loss w.r.t. the sample these schedulers take does not exist (the reference's torch.autograd.grad(rec_loss, "
                               "sample) raises for it, scheduling_dps.py:212)")
        t, a_t, a_p, sigma = self._scalars(timestep, eta)
        x = sample.detach().to(torch.float32).contiguous()
        e = model_output.detach().to(torch.float32).contiguous()
        # epsilon prediction without clipping (ptype 0, clip_r 0: the reference's configs) or the DDIM parent's other branches (sample /
        # v_prediction, clip_sample)
        x0 = ops.hip.sched_pred_x0(x, e, a_t, ptype=self._ptype, clip_r=self._clip_r)
        mode = _MODE[self.mode]
        noise = None
        if self.mode in ("dps", "mpgd") and eta > 0:
            if variance_noise is None:
                if self.passes_eta_to_parent:          # keep the reference's RNG stream
                    randn_tensor(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
                variance_noise = randn_tensor(model_output.shape, generator=generator, device=model_output.device,
                                              dtype=model_output.dtype)
            noise = variance_noise.to(torch.float32).contiguous()
        loss = g0 = inv_scale = None
        if self.mode == "ddim":
            loss = torch.tensor([t])
        else:
            loss, g0, inv_scale = self._guidance(x0, measurement, vae, vocoder, original_waveform_length, supervised_space,
                                                 self._op_kwargs(kwargs.get("op_kwargs"), t, generator))
            if self.mode in ("dsg", "diffmusic"):
                sn = kwargs.get("sample_noise")
                if sn is None and self.device_noise:
                    sn = self._philox_noise(model_output.shape, generator, model_output.device)
                elif sn is None:
                    sn = randn_tensor(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
                noise = sn.to(torch.float32).contiguous()
        grad_out = torch.empty_like(x) if self.debug_keep_grad and self.mode != "ddim" else None
        upd = (mode, x, e, x0, g0, inv_scale, noise, a_t, a_p, sigma, float(rate), float(eps), not self.per_clip_norm)
        with stage("sched_update"):
            # x0_out: MPGD's guided x0, None for every other mode
            prev, x0_out = ops.hip.sched_update(*upd, ptype=self._ptype, clip_r=self._clip_r, grad_out=grad_out)
        self.last_grad = grad_out
        if loss.numel() == 1 and self.mode != "ddim":
            loss = loss.reshape(())
        return InverseProblemSchedulerOutput(prev_sample=prev.to(sample.dtype),
                                             pred_original_sample=(x0_out if x0_out is not None else x0).to(sample.dtype),
                                             loss=loss)

    def _philox_noise(self, shape, generator, device):
        gens = generator if isinstance(generator, (list, tuple)) else [generator] * shape[0]
        if any(g is None for g in gens):
            raise ValueError("device_noise=True needs generator(s): their initial seeds key the per-clip Philox streams")
        seeds = [int(g.initial_seed()) + (0 if isinstance(generator, (list, tuple)) else i) for i, g in enumerate(gens)]
        n = 1
        for d in shape[1:]:
            n *= int(d)
        out = randn_philox(shape, seeds, self._noise_offset, device)
        self._noise_offset += (n + 3) // 4
        return out

    def optim_prompt(self, model_output, timestep, sample, encoder_hidden_states=None, encoder_hidden_states_1=None, eta=0.0,
                     use_clipped_model_output=False, generator=None, variance_noise=None, return_dict=True, measurement=None,
                     vae=None, vocoder=None, original_waveform_length=0, optim_prompt_learning_rate=1e-4,
                     supervised_space="mel_spectrogram", *args, **kwargs):
        """`optim_prompt` of the reference (scheduling_dps.py:63-135 and siblings): meant to be one SGD step on the prompt
        embeddings, but the `requires_grad_` clones it makes (:93-96) are discarded and `model_output` was computed from the
        originals, so no gradient ever reaches the embeddings -- the call returns them unchanged.  Reproduced as that no-op
        (same signature, same output fields, same argument validation); the pipeline calls it every `t % 30 == 1` when
        `optim_prompt=True` (pipeline_musicldm.py:710-723)."""
        if supervised_space not in ("wav_form", "mel_spectrogram"):
            raise ValueError("supervised_space should be either 'wav_form' or 'mel_spectrogram")
        d = lambda v: v.detach() if v is not None else None          # noqa: E731  (the reference crashes on None here, :132)
        return InverseProblemSchedulerOutput(encoder_hidden_states=d(encoder_hidden_states),
                                             encoder_hidden_states_1=d(encoder_hidden_states_1))


class DDIMScheduler(GuidedDDIMScheduler):        # scheduling_ddim.py:58-104 (the formula; the reference body crashes)
    mode = "ddim"


class DPSScheduler(GuidedDDIMScheduler):         # scheduling_dps.py:137-219
    mode, default_eta, default_rate, passes_eta_to_parent = "dps", 0.0, 5e-4, True


class MPGDScheduler(GuidedDDIMScheduler):        # scheduling_mpgd.py:137-224
    mode, default_eta, default_rate, passes_eta_to_parent = "mpgd", 0.0, 1.0, True


class DSGScheduler(GuidedDDIMScheduler):         # scheduling_dsg.py:148-230
    mode, default_eta, default_rate = "dsg", 1.0, 0.08


class DiffMusicScheduler(GuidedDDIMScheduler):   # scheduling_diffmusic.py:148-229
    mode, default_eta, default_rate = "diffmusic", 0.0, 0.08
