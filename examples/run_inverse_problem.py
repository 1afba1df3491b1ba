#!/usr/bin/env python
"""End-to-end driver for one inverse problem on the MI355X engine: the output stage of SURVEY.md section 8f row 1.

Follows the flow of the reference's run.py (:147-220 operator / scheduler / pipeline wiring, :317-370 call and
outputs) on the three registries of this package.  The text encoders are out of scope, so the prompt conditioning is an
embedding file (`--prompt_embeds x.npy`, (B, 512) CLAP text embeddings for MusicLDM) or a seeded unit vector.

    python examples/run_inverse_problem.py -c dps -t music_inpainting --wav a.wav b.wav --weights /ckpt/musicldm
    python examples/run_inverse_problem.py -c mpgd -t super_resolution --num_inference_steps 20      # synthetic clips + weights
    python examples/run_inverse_problem.py -c dps -t music_dereverberation --wav take.wav --track_overlap_s 1.28   # a long take, whole
    python examples/run_inverse_problem.py -c dps -t music_declipping --clip_sdr_db 3 --init measurement --strength 0.5 --project
    python examples/run_inverse_problem.py -c dps -t music_blind_dereverberation --wav room.wav        # the response is fitted, not given
    python examples/run_inverse_problem.py -c dps -t music_source_separation --wav drums.wav bass.wav --gains 1 0.5 --project
    python examples/run_inverse_problem.py -c dps -t music_source_separation --mixture song.wav --stems 4 --track_overlap_s 1.28
    python examples/run_inverse_problem.py -c dps -t music_spectral_inpainting --tf_box 2000,4000,2,2.5 --hum 50,5      # a spectral hole + hum
    python examples/run_inverse_problem.py -c dps -t music_blind_equalization --eq_lowpass 3000,4      # the EQ curve is fitted, not given
    python examples/run_inverse_problem.py -c dps -t music_decompression --drc_threshold_db -30 --drc_ratio inf      # undo a limiter
    python examples/run_inverse_problem.py -c dps -t music_wow_flutter --wow 0.5,1 --wow 9,0.2 --speed_pct 0.5      # wow, flutter and a drift
    python examples/run_inverse_problem.py -c dps -t music_declicking --clicks_per_s 20 --supervised_space wav_form --project   # a crackly side

`--track_overlap_s S` restores a recording longer than the model window whole (track mode, inverse_problem/track.py): the first `--wav`
(or a synthetic 2.5-window signal) becomes overlapping windows under one loss and one stitched file is written.  Without the flag a
long `--wav` is cropped to the window as before.

`-t music_spectral_inpainting` measures through a gain on the spectrogram (TimeFrequencyMaskOperator): `--tf_box f_lo,f_hi,t0,t1[,gain]`
(Hz and seconds, an empty field = to the edge, gain 0 by default; repeatable, later boxes overwrite earlier ones) and `--hum
f0[,harmonics[,width]]`; without either flag the boxes of configs/inverse_problem/music_spectral_inpainting.yaml are used.

`-t music_blind_equalization` measures through an equalisation curve that the restoration does not know (BlindEqualizationOperator fits
it inside the guided loop): `--eq_lowpass HZ[,ORDER]` (a Butterworth magnitude, order 4 by default) or `--eq_points "f,dB;f,dB;..."`
(breakpoints, linear in dB over log-frequency) is the TRUE curve of the synthetic measurement; the two exclude each other, and without
either the `points` of configs/inverse_problem/music_blind_equalization.yaml are used.

`-t music_decompression` measures through a dynamic-range compressor with given parameters (DynamicRangeOperator): `--drc_threshold_db`,
`--drc_ratio` (>= 1, `inf` = a limiter), `--drc_knee_db`, `--drc_attack_ms`, `--drc_release_ms`, `--drc_makeup_db`; a flag that is not
given takes its value from configs/inverse_problem/music_decompression.yaml.

`-t music_wow_flutter` measures through a playback speed that was off and varied (TimeWarpOperator; the delay curve is given, not fitted):
`--wow RATE_HZ,DEPTH_PCT[,PHASE_DEG]` (repeatable: one speed-modulation component each) and `--speed_pct P` (a constant speed error);
a flag that is not given takes its value from configs/inverse_problem/music_wow_flutter.yaml.  The curve is built for the clip's length,
in track mode for the track's.

`-t music_declicking` restores a recording with impulsive noise (DeclickOperator: clicks are detected from the measurement and hidden from
the loss): `--clicks_per_s R` and `--click_amp LO,HI` shape the synthetic measurement's clicks, `--declick_threshold K` and `--declick_guard G`
the detector; a flag that is not given takes its value from configs/inverse_problem/music_declicking.yaml.  `--project` keeps the
measurement's own samples away from the detected clicks (meaningful with `--supervised_space wav_form`); the masked fraction is printed.

`-t music_blind_wow_flutter` measures through the same kind of curve, which the restoration does not know (BlindTimeWarpOperator fits it
inside the guided loop): `--wow` / `--speed_pct` build the TRUE curve of the synthetic measurement, `--warp_knot_stride S` (fine knots
per coarse knot of the estimate, a power of two up to 64), `--warp_max_delay M` (samples, at most min(4096, 8 S)) and `--warp_lr`
(samples per step) shape the fit; a flag that is not given takes its value from configs/inverse_problem/music_blind_wow_flutter.yaml.

`-t music_blind_decompression` measures through a compressor whose settings the restoration does not know (BlindDynamicRangeOperator fits
them inside the guided loop): the `--drc_*` flags above are the TRUE parameters of the synthetic measurement (`--drc_knee_db` is the knee
width both sides share: it is given, not fitted), `--drc_fit threshold,ratio,makeup[,attack,release]` names the parameters that move, and
`--drc_init_threshold_db`, `--drc_init_ratio`, `--drc_init_attack_ms`, `--drc_init_release_ms`, `--drc_init_makeup_db` say where the fit
starts; a flag that is not given takes its value from configs/inverse_problem/music_blind_decompression.yaml.

`-t music_codec_restoration` measures through an MDCT quantiser (CodecOperator: the coefficients of a lossy codec, one step per band and
frame, nothing above the cut-off): `--codec_nmr_db X` chooses the steps a codec's rate loop would, X dB of noise-to-mask ratio below every
band of the clean clip, `--codec_step_db X` a fixed grid instead (the step at 1 kHz in dB re 1.0; the two exclude each other), and
`--codec_cutoff_hz F` the low-pass; a flag that is not given takes its value from configs/inverse_problem/music_codec_restoration.yaml.
The grid is built for the clip's length, in track mode for the track's.  `--project` clamps the result's coefficients into the quantiser
cells of the measurement's own codes (meaningful with `--supervised_space wav_form`).

`-t music_source_separation` restores K stems from their mixture under one loss (inverse_problem/mixture.py), one prompt embedding per
stem: `--wav` names the stems whose gain-weighted sum (`--gains`) is the measurement (SI-SDR per stem is printed), `--mixture mix.wav
--stems K` separates a real mixture.  One file per stem is written; `--project` makes the stems sum to the mixture exactly.
"""
import argparse
import math
import os
import sys
from pathlib import Path

import numpy as np
import scipy.io.wavfile
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from diffmusic_amd.config import compose                                            # noqa: E402
from diffmusic_amd import inverse_problem as P                                      # noqa: E402
from diffmusic_amd.metrics import LogSpectralDistance, MeanSquaredError, ScaleInvariantSDR   # noqa: E402
from diffmusic_amd.pipelines import get_pipeline                                    # noqa: E402
from diffmusic_amd.schedulers import get_scheduler                                  # noqa: E402

TASKS = ("music_generation", "music_inpainting", "super_resolution", "phase_retrieval", "music_dereverberation", "music_declipping",
         "music_blind_dereverberation", "music_source_separation", "music_spectral_inpainting", "music_blind_equalization", "music_decompression",
         "music_wow_flutter", "music_blind_wow_flutter", "music_blind_decompression", "music_declicking", "music_codec_restoration")
SEPARATION = "music_source_separation"
SPECTRAL = "music_spectral_inpainting"
BLIND_EQ = "music_blind_equalization"
DECOMPRESSION = "music_decompression"
WOW_FLUTTER = "music_wow_flutter"
BLIND_WOW = "music_blind_wow_flutter"
BLIND_DRC = "music_blind_decompression"
DECLICK = "music_declicking"
CODEC = "music_codec_restoration"
DRC_INIT_FLAGS = ("threshold_db", "ratio", "attack_ms", "release_ms", "makeup_db")
DRC_FLAGS = ("threshold_db", "ratio", "knee_db", "attack_ms", "release_ms", "makeup_db")


def build_operator(task, cfg, mask_type, audio_length_in_s=None, clip_threshold=None, tf_boxes=None, eq_true=None, drc=None, warp=None,
                   blind_warp=None, blind_drc=None, declick=None, codec=None, codec_audio=None):
    """run.py:157-212: one operator per task, constructor arguments from the data / model config.  `audio_length_in_s`: the length the
    operator acts on when it is not the model window (a track).  `clip_threshold`: music_declipping's threshold(s), a float or one value
    per clip (`threshold_for_sdr` of the clean clips).  `tf_boxes`: music_spectral_inpainting's boxes (`spectral_boxes`).  `eq_true`:
    music_blind_equalization's true curve (`equalization_curve`), kept on the operator for `forward`.  `drc`: music_decompression's
    parameters (`compressor_params`).  `warp`: music_wow_flutter's speed components (`warp_params`); the delay curve is built here, for the
    length the operator acts on.  `blind_warp`: music_blind_wow_flutter's fit options (`blind_warp_params`); `warp` then describes the TRUE
    curve, kept on the operator for `forward`.  `blind_drc`: music_blind_decompression's `operator` keyword arguments and the `true`
    parameters of the measurement (`blind_drc_params`), the latter kept on the operator for `forward`.  `codec`: music_codec_restoration's
    grid recipe (`codec_params`); with `nmr_db` the steps follow `codec_audio`, the clean clips (B, L) or the one track (L,), and the grid
    is built for their length."""
    noiser = P.get_noiser(**cfg.inverse_problem.noise)
    d, scale = cfg.data, 1
    seconds = cfg.model.pipe.audio_length_in_s if audio_length_in_s is None else audio_length_in_s
    if task == "music_generation":
        op = P.IdentityOperator(sample_rate=d.sample_rate)
    elif task == "music_inpainting":
        op = P.MusicInpaintingOperator(audio_length_in_s=seconds, sample_rate=d.sample_rate, mask_type=mask_type,
                                       start_inpainting_s=d.start_inpainting_s - d.start_s, end_inpainting_s=d.end_inpainting_s - d.start_s,
                                       mask_percentage=0.3, interval_s=1, mask_duration_s=0.1, noiser=noiser)
    elif task == "super_resolution":
        scale = 2
        op = P.SuperResolutionOperator(sample_rate=d.sample_rate, scale=scale, noiser=noiser)
    elif task == "phase_retrieval":
        op = P.PhaseRetrievalOperator(n_fft=d.n_fft, hop_length=d.hop_length, win_length=d.win_length, noiser=noiser)
    elif task == "music_dereverberation":
        op = P.MusicDereverberationOperator(ir_length=5000, decay_factor=0.99, noiser=noiser)
    elif task == "music_blind_dereverberation":
        op = P.BlindDereverberationOperator(ir_length=5000, decay_factor=0.99, noiser=noiser, lr=cfg.inverse_problem.get("lr") or 0.05)
    elif task == "music_declipping":
        if clip_threshold is None:
            raise ValueError("music_declipping needs clip_threshold (e.g. inverse_problem.threshold_for_sdr(clean, sdr_db))")
        op = P.DeclippingOperator(sample_rate=d.sample_rate, threshold=clip_threshold, noiser=noiser)
    elif task == SPECTRAL:
        if tf_boxes is None:
            raise ValueError("music_spectral_inpainting needs tf_boxes (spectral_boxes(args, cfg))")
        grid = P.tf_gain_grid(int(seconds * d.sample_rate), d.sample_rate, tf_boxes, base=float(cfg.inverse_problem.get("base", 1.0)))
        op = P.TimeFrequencyMaskOperator(sample_rate=d.sample_rate, gain=grid, noiser=noiser)
    elif task == BLIND_EQ:
        if eq_true is None:
            raise ValueError("music_blind_equalization needs eq_true (equalization_curve(args, cfg))")
        ip = cfg.inverse_problem
        op = P.BlindEqualizationOperator(sample_rate=d.sample_rate, noiser=noiser, lr=ip.get("lr") or 0.05,
                                         betas=tuple(ip.get("betas") or (0.9, 0.999)), adam_eps=float(ip.get("adam_eps") or 1e-8),
                                         init=ip.get("init") or "flat", normalize=ip.get("normalize") or "peak")
        op.true_curve = torch.as_tensor(np.asarray(eq_true, dtype=np.float32)).reshape(1, -1)
    elif task == DECOMPRESSION:
        if drc is None:
            raise ValueError("music_decompression needs drc (compressor_params(args, cfg))")
        op = P.DynamicRangeOperator(sample_rate=d.sample_rate, noiser=noiser, **drc)
    elif task == WOW_FLUTTER:
        if warp is None:
            raise ValueError("music_wow_flutter needs warp (warp_params(args, cfg))")
        curve = P.wow_curve(int(seconds * d.sample_rate), d.sample_rate, **warp)
        op = P.TimeWarpOperator(sample_rate=d.sample_rate, delay=curve, noiser=noiser)
    elif task == BLIND_WOW:
        if warp is None or blind_warp is None:
            raise ValueError("music_blind_wow_flutter needs warp (warp_params(args, cfg)) and blind_warp (blind_warp_params(args, cfg))")
        ip = cfg.inverse_problem
        op = P.BlindTimeWarpOperator(sample_rate=d.sample_rate, noiser=noiser, betas=tuple(ip.get("betas") or (0.9, 0.999)),
                                     adam_eps=float(ip.get("adam_eps") or 1e-8), init=ip.get("init") or "zero",
                                     anchor=ip.get("anchor") or "mean", **blind_warp)
        op.true_delay = torch.from_numpy(P.wow_curve(int(seconds * d.sample_rate), d.sample_rate, **warp)).reshape(1, -1)
    elif task == BLIND_DRC:
        if blind_drc is None:
            raise ValueError("music_blind_decompression needs blind_drc (blind_drc_params(args, cfg))")
        op = P.BlindDynamicRangeOperator(sample_rate=d.sample_rate, noiser=noiser, **blind_drc["operator"])
        op.true_params = dict(blind_drc["true"])
    elif task == DECLICK:
        if declick is None:
            raise ValueError("music_declicking needs declick (declick_params(args, cfg))")
        op = P.DeclickOperator(sample_rate=d.sample_rate, noiser=noiser, **declick["operator"])
        op.click_recipe = dict(declick["clicks"])              # the synthetic measurement's clicks (`synthetic_clicks`)
    elif task == CODEC:
        if codec is None:
            raise ValueError("music_codec_restoration needs codec (codec_params(args, cfg))")
        if codec.get("nmr_db") is not None:
            if codec_audio is None:
                raise ValueError("music_codec_restoration with nmr_db needs codec_audio, the clean audio the steps adapt to")
            audio = torch.as_tensor(codec_audio).detach().cpu().numpy()
            grid = P.codec_steps_for_nmr(audio, d.sample_rate, codec["nmr_db"], cutoff_hz=codec.get("cutoff_hz"))
        else:
            grid = P.codec_step_grid(int(seconds * d.sample_rate), d.sample_rate, codec["step_db"], cutoff_hz=codec.get("cutoff_hz"),
                                     tilt_db_per_octave=codec.get("tilt_db_per_octave", 0.0))
        op = P.CodecOperator(sample_rate=d.sample_rate, step=grid, noiser=noiser)
    else:
        raise ValueError(f"Unknown task: {task}")
    return op, scale


def codec_params(args, cfg):
    """The argument rules of -t music_codec_restoration -> {"nmr_db" or "step_db", "cutoff_hz", "tilt_db_per_octave"}: --codec_nmr_db and
    --codec_step_db exclude each other and replace BOTH of the config's; --codec_cutoff_hz (0 or less: no cut-off) replaces the config's.
    Exactly one of nmr_db / step_db must remain.  Any other task refuses the flags."""
    flags = dict(codec_nmr_db=args.codec_nmr_db, codec_step_db=args.codec_step_db, codec_cutoff_hz=args.codec_cutoff_hz)
    if args.task != CODEC:
        for name, v in flags.items():
            if v is not None:
                raise SystemExit(f"--{name} belongs to -t {CODEC}")
        return None
    if args.codec_nmr_db is not None and args.codec_step_db is not None:
        raise SystemExit("--codec_nmr_db (signal-adaptive steps) and --codec_step_db (a fixed grid) exclude each other")
    ip = cfg.inverse_problem
    nmr, step = ip.get("nmr_db"), ip.get("step_db")
    if args.codec_nmr_db is not None:
        nmr, step = args.codec_nmr_db, None
    elif args.codec_step_db is not None:
        nmr, step = None, args.codec_step_db
    if (nmr is None) == (step is None):
        raise SystemExit(f"-t {CODEC}: exactly one of nmr_db / step_db (--codec_nmr_db / --codec_step_db)")
    cutoff = ip.get("cutoff_hz") if args.codec_cutoff_hz is None else (args.codec_cutoff_hz if args.codec_cutoff_hz > 0 else None)
    out = dict(cutoff_hz=None if cutoff is None else float(cutoff), tilt_db_per_octave=float(ip.get("tilt_db_per_octave") or 0.0))
    out["nmr_db" if nmr is not None else "step_db"] = float(nmr if nmr is not None else step)
    try:
        if nmr is not None:
            P.codec_steps_for_nmr(np.zeros(16), cfg.data.sample_rate, out["nmr_db"], cutoff_hz=out["cutoff_hz"])
        else:
            P.codec_step_grid(16, cfg.data.sample_rate, out["step_db"], cutoff_hz=out["cutoff_hz"], tilt_db_per_octave=out["tilt_db_per_octave"])
    except ValueError as e:
        raise SystemExit(f"-t {CODEC}: {e}")
    return out


def declick_params(args, cfg):
    """The argument rules of -t music_declicking -> {"operator": the DeclickOperator's `threshold`, `sigma_floor` and `guard`, "clicks":
    the `rate_hz`, `amplitude`, `max_width` and `seed` of `dsp.click_train`}: --declick_threshold, --declick_guard, --clicks_per_s and
    --click_amp LO,HI, else the task's config.  The operator's own refusals come before any GPU work.  Any other task refuses the flags."""
    flags = dict(clicks_per_s=args.clicks_per_s, click_amp=args.click_amp, declick_threshold=args.declick_threshold, declick_guard=args.declick_guard)
    if args.task != DECLICK:
        for name, v in flags.items():
            if v is not None:
                raise SystemExit(f"--{name} belongs to -t {DECLICK}")
        return None
    ip = cfg.inverse_problem
    c = dict(ip.get("clicks") or {})
    amp = tuple(float(v) for v in (c.get("amplitude") or (0.3, 0.6)))
    if args.click_amp is not None:
        try:
            amp = tuple(float(v) for v in args.click_amp.split(","))
        except ValueError:
            amp = ()
        if len(amp) != 2:
            raise SystemExit(f"--click_amp {args.click_amp!r}: LO,HI")
    out = {"operator": dict(threshold=float(args.declick_threshold if args.declick_threshold is not None else ip.get("threshold", 5.0)),
                            sigma_floor=float(ip.get("sigma_floor", 1e-5)),
                            guard=int(args.declick_guard if args.declick_guard is not None else ip.get("guard", 3))),
           "clicks": dict(rate_hz=float(args.clicks_per_s if args.clicks_per_s is not None else c.get("rate_hz", 20.0)), amplitude=amp,
                          max_width=int(c.get("max_width", 3)), seed=int(c.get("seed", 0)))}
    try:
        P.DeclickOperator(**out["operator"])
        P.click_train(16, cfg.data.sample_rate, **out["clicks"])
    except ValueError as e:
        raise SystemExit(f"-t {DECLICK}: {e}")
    return out


def synthetic_clicks(op, gt, sample_rate):
    """The clicks of a synthetic declicking measurement, shaped like `gt`, from the recipe `build_operator` left on the operator."""
    return P.click_train(gt.shape[1], sample_rate, batch=gt.shape[0], **op.click_recipe).to(gt.device)


# why the measurement of a task cannot seed a warm start (the encoder takes a full-rate waveform of the clip's length)
NO_WARM_START = dict(super_resolution="its measurement is sampled at 1 / scale of the model's rate",
                     phase_retrieval="its measurement is an STFT magnitude, not a waveform")


def init_from_measurement(task, measurement, length):
    if task in NO_WARM_START:
        raise SystemExit(f"--init measurement is not available for {task}: {NO_WARM_START[task]}")
    if measurement.dim() != 2 or measurement.shape[1] < length:
        raise SystemExit(f"--init measurement needs a (B, >= {length}) waveform, the measurement is {tuple(measurement.shape)}")
    return measurement


def load_clips(paths, n, sr, length, seed, start_s=0.0, whole=False):
    """(B, length) fp32 in [-1, 1]: wav files decoded, mixed down to mono and resampled to `sr` by the dataset loader
    (diffmusic_amd/data/dataloader.py; reference dataloader.py:47-89), cropped from `start_s` / zero-padded to `length`;
    seeded synthetic chords fill up to `n`.  whole=True (track mode): the first file uncropped, or 2.5 windows of chords, as (1, T)."""
    if whole:
        paths, n = paths[:1], 1
    from diffmusic_amd.data.dataloader import load_wav
    from diffmusic_amd.pipelines.prompt_audioldm2 import resample_to
    clips = []
    for p in paths:
        x, rate = load_wav(p)
        x = x.mean(dim=0, keepdim=True)
        if rate != sr:
            x = resample_to(x, rate, sr)
        x = x[0, int(start_s * sr):]
        x = x if whole else x[:length]
        clips.append(torch.nn.functional.pad(x, (0, max(0, length - x.numel()))))
    g = torch.Generator().manual_seed(seed)
    if whole and not clips:
        length = 5 * length // 2
    while len(clips) < n:
        f = 110.0 * 2 ** (torch.randint(0, 36, (4,), generator=g).float() / 12)
        t = torch.arange(length, dtype=torch.float32) / sr
        clips.append(0.2 * torch.sin(2 * math.pi * f[:, None] * t[None]).sum(0).clamp(-1, 1))
    return torch.stack(clips[:max(n, len(paths))])


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-c", "--config_name", default="dps", choices=["ddim", "dps", "mpgd", "dsg", "diffmusic"])
    ap.add_argument("-t", "--task", default="music_inpainting", choices=TASKS)
    ap.add_argument("-m", "--model", default="musicldm", choices=["musicldm", "audioldm2"])
    ap.add_argument("--data", default="moises")
    ap.add_argument("--mask_type", default="box", choices=["box", "random", "periodic"])
    ap.add_argument("--supervised_space", default="mel_spectrogram")
    ap.add_argument("--weights", default="synthetic", help="checkpoint directory with {unet,vae,vocoder}/*.safetensors, or 'synthetic'")
    ap.add_argument("--wav", nargs="*", default=[], help="input clips (any PCM / float wav: mixed to mono and resampled to the data sample rate); synthetic clips fill up to --batch")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--prompt_embeds", default=None, help=".npy with (B, 512) text embeddings (MusicLDM)")
    ap.add_argument("--num_inference_steps", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--output_dir", default="outputs")
    ap.add_argument("--show_progress", action="store_true")
    ap.add_argument("--init", default="none", choices=["none", "measurement"],
                    help="warm start: encode the measurement, noise it to an intermediate timestep and run only the last steps (--strength)")
    ap.add_argument("--track_overlap_s", type=float, default=None,
                    help="track mode: restore the first --wav whole as overlapping model windows under one loss, with this overlap in seconds")
    ap.add_argument("--clip_sdr_db", type=float, default=3.0,
                    help="music_declipping: input SDR in dB of the clipped measurement (each clip's threshold is found from it)")
    ap.add_argument("--project", action="store_true",
                    help="music_declipping: finish with the consistency projection (measurement kept where it is unclipped)")
    ap.add_argument("--gains", type=float, nargs="*", default=None, help="music_source_separation: one mixing gain per stem (default: all 1)")
    ap.add_argument("--mixture", default=None, help="music_source_separation: a real mixture to separate (then --stems K, no --wav)")
    ap.add_argument("--stems", type=int, default=None, help="music_source_separation: number of stems K (default: the number of --wav, else 2)")
    ap.add_argument("--tf_box", action="append", default=None, metavar="F_LO,F_HI,T0,T1[,GAIN]",
                    help="music_spectral_inpainting: a box of the spectrogram (Hz, seconds; empty field = to the edge) set to GAIN (default 0); repeatable")
    ap.add_argument("--hum", default=None, metavar="F0[,HARMONICS[,WIDTH]]",
                    help="music_spectral_inpainting: remove bands of WIDTH Hz (default 32) around F0 .. HARMONICS * F0 (default 1)")
    ap.add_argument("--eq_lowpass", default=None, metavar="HZ[,ORDER]",
                    help="music_blind_equalization: the true curve is a Butterworth low-pass magnitude at HZ (ORDER 4 by default)")
    ap.add_argument("--eq_points", default=None, metavar="F,DB;F,DB;...",
                    help="music_blind_equalization: the true curve through (Hz, dB) breakpoints, linear in dB over log-frequency")
    for flag, what in zip(DRC_FLAGS, ("threshold in dB", "ratio >= 1, inf = a limiter", "knee width in dB, 0 = hard knee", "attack time in ms",
                                      "release time in ms", "make-up gain in dB")):
        ap.add_argument(f"--drc_{flag}", type=float, default=None, help=f"music_decompression: the compressor's {what} (default: the task's config)")
    ap.add_argument("--drc_fit", default=None, metavar="NAME,NAME,...",
                    help="music_blind_decompression: the parameters that are fitted, of threshold, ratio, makeup, attack, release "
                         "(default: the task's config)")
    for flag in DRC_INIT_FLAGS:
        ap.add_argument(f"--drc_init_{flag}", type=float, default=None,
                        help=f"music_blind_decompression: where the fit of {flag} starts (default: the task's config)")
    ap.add_argument("--clicks_per_s", type=float, default=None, help="music_declicking: clicks per second of the synthetic measurement (default: the task's config)")
    ap.add_argument("--click_amp", default=None, metavar="LO,HI", help="music_declicking: the clicks' amplitude range (default: the task's config)")
    ap.add_argument("--declick_threshold", type=float, default=None,
                    help="music_declicking: a residual above this multiple of the frame's robust scale is a click (default: the task's config)")
    ap.add_argument("--declick_guard", type=int, default=None,
                    help="music_declicking: samples hidden on each side of a detected one, 0 .. 64 (default: the task's config)")
    ap.add_argument("--codec_nmr_db", type=float, default=None,
                    help="music_codec_restoration: signal-adaptive steps, the quantisation noise this many dB below each band (default: the task's config)")
    ap.add_argument("--codec_step_db", type=float, default=None,
                    help="music_codec_restoration: a fixed step grid instead, the step at 1 kHz in dB re 1.0 (default: the task's config)")
    ap.add_argument("--codec_cutoff_hz", type=float, default=None,
                    help="music_codec_restoration: coefficients above this frequency are discarded, 0 = none (default: the task's config)")
    ap.add_argument("--wow", action="append", default=None, metavar="RATE_HZ,DEPTH_PCT[,PHASE_DEG]",
                    help="music_wow_flutter: one speed-modulation component (repeatable; default: the task's config)")
    ap.add_argument("--speed_pct", type=float, default=None, help="music_wow_flutter: constant speed error in percent (default: the task's config)")
    ap.add_argument("--warp_knot_stride", type=int, default=None,
                    help="music_blind_wow_flutter: fine knots per coarse knot of the estimate, a power of two up to 64 (default: the task's config)")
    ap.add_argument("--warp_max_delay", type=float, default=None,
                    help="music_blind_wow_flutter: the clamp of every knot in samples, at most min(4096, 8 * knot_stride) (default: the task's config)")
    ap.add_argument("--warp_lr", type=float, default=None, help="music_blind_wow_flutter: Adam step of the curve in samples (default: the task's config)")
    ap.add_argument("--strength", type=float, default=1.0, help="share of num_inference_steps a warm start runs (diffusers' img2img rule)")
    return ap.parse_args(argv)


def _field(text, what):
    text = text.strip()
    if text == "" or text.lower() == "none":
        return None
    try:
        v = float(text)
    except ValueError:
        raise SystemExit(f"{what}: {text!r} is not a number")
    if not math.isfinite(v):
        raise SystemExit(f"{what}: {text!r} is not finite")
    return v


def spectral_boxes(args, cfg=None):
    """The argument rules of -t music_spectral_inpainting -> the boxes of `tf_gain_grid`, in order: --hum first, then every --tf_box; with
    neither flag, the `hum` and `boxes` of the task's config.  Any other task refuses the two flags."""
    if args.task != SPECTRAL:
        for flag in ("tf_box", "hum"):
            if getattr(args, flag) is not None:
                raise SystemExit(f"--{flag} belongs to -t {SPECTRAL}")
        return None
    boxes = []
    hum, tf_box = args.hum, args.tf_box
    if hum is None and tf_box is None and cfg is not None:
        ip = cfg.inverse_problem
        hum = ",".join(str(v) for v in ip.get("hum")) if ip.get("hum") else None
        tf_box = [",".join("" if v is None else str(v) for v in b) for b in (ip.get("boxes") or [])]
    if hum is not None:
        parts = hum.split(",")
        if not 1 <= len(parts) <= 3:
            raise SystemExit(f"--hum {hum}: F0[,HARMONICS[,WIDTH]]")
        vals = [_field(p, "--hum") for p in parts]
        if vals[0] is None or vals[0] <= 0:
            raise SystemExit(f"--hum {hum}: F0 is a positive frequency in Hz")
        harmonics = 1 if len(vals) < 2 or vals[1] is None else vals[1]
        if harmonics != int(harmonics) or harmonics < 1:
            raise SystemExit(f"--hum {hum}: HARMONICS is a whole number >= 1")
        width = 32.0 if len(vals) < 3 or vals[2] is None else vals[2]
        if width < 0:
            raise SystemExit(f"--hum {hum}: WIDTH is a width in Hz, >= 0")
        boxes += P.hum_boxes(vals[0], int(harmonics), width)
    for text in tf_box or []:
        parts = text.split(",")
        if len(parts) not in (4, 5):
            raise SystemExit(f"--tf_box {text}: F_LO,F_HI,T0,T1[,GAIN]")
        f_lo, f_hi, t0, t1 = (_field(p, "--tf_box") for p in parts[:4])
        gain = _field(parts[4], "--tf_box") if len(parts) == 5 else 0.0
        if gain is None:
            raise SystemExit(f"--tf_box {text}: GAIN is a number")
        if f_lo is not None and f_hi is not None and f_lo > f_hi:
            raise SystemExit(f"--tf_box {text}: F_LO > F_HI")
        if t0 is not None and t1 is not None and t0 >= t1:
            raise SystemExit(f"--tf_box {text}: T0 >= T1")
        boxes.append((f_lo, f_hi, t0, t1, gain))
    if not boxes:
        raise SystemExit(f"-t {SPECTRAL} needs at least one --tf_box or --hum (or boxes in its config)")
    return boxes


def equalization_curve(args, cfg=None):
    """The argument rules of -t music_blind_equalization -> the true (513,) curve of the synthetic measurement: --eq_lowpass or
    --eq_points (not both); with neither, the `points` of the task's config.  Any other task refuses the two flags."""
    if args.task != BLIND_EQ:
        for flag in ("eq_lowpass", "eq_points"):
            if getattr(args, flag) is not None:
                raise SystemExit(f"--{flag} belongs to -t {BLIND_EQ}")
        return None
    if args.eq_lowpass is not None and args.eq_points is not None:
        raise SystemExit("--eq_lowpass and --eq_points both name the true curve: pass one of them")
    sr = 16000 if cfg is None else cfg.data.sample_rate
    if args.eq_lowpass is not None:
        parts = args.eq_lowpass.split(",")
        if not 1 <= len(parts) <= 2:
            raise SystemExit(f"--eq_lowpass {args.eq_lowpass}: HZ[,ORDER]")
        vals = [_field(p, "--eq_lowpass") for p in parts]
        if vals[0] is None or vals[0] <= 0:
            raise SystemExit(f"--eq_lowpass {args.eq_lowpass}: HZ is a positive frequency")
        order = 4 if len(vals) < 2 or vals[1] is None else vals[1]
        if order != int(order) or order < 1:
            raise SystemExit(f"--eq_lowpass {args.eq_lowpass}: ORDER is a whole number >= 1")
        return P.lowpass_curve(sr, vals[0], int(order))
    if args.eq_points is not None:
        points = []
        for text in args.eq_points.split(";"):
            parts = text.split(",")
            if len(parts) != 2:
                raise SystemExit(f"--eq_points {args.eq_points}: F,DB;F,DB;...")
            f, db = (_field(p, "--eq_points") for p in parts)
            if f is None or db is None or f <= 0:
                raise SystemExit(f"--eq_points {args.eq_points}: every point is a positive frequency in Hz and a gain in dB")
            points.append((f, db))
    else:
        points = [tuple(p) for p in ((cfg.inverse_problem.get("points") if cfg is not None else None) or [])]
        if not points:
            raise SystemExit(f"-t {BLIND_EQ} needs --eq_lowpass or --eq_points (or points in its config)")
    if any(b[0] <= a[0] for a, b in zip(points, points[1:])):
        raise SystemExit("--eq_points: the frequencies increase strictly")
    return P.eq_curve(sr, points)


def compressor_params(args, cfg=None):
    """The argument rules of -t music_decompression -> the keyword arguments of the DynamicRangeOperator: every --drc_* flag that is given,
    the task's config for the others (the operator's defaults without a config).  argparse's float reads `inf`; the operator refuses a bad
    value by name.  Any other task refuses the flags."""
    given = {flag: getattr(args, f"drc_{flag}") for flag in DRC_FLAGS if getattr(args, f"drc_{flag}") is not None}
    if args.task != DECOMPRESSION:
        if given and args.task != BLIND_DRC:                                       # there they describe the measurement (blind_drc_params)
            raise SystemExit(f"--drc_{next(iter(given))} belongs to -t {DECOMPRESSION} and -t {BLIND_DRC}")
        return None
    out = {}
    if cfg is not None:
        out = {flag: float(cfg.inverse_problem.get(flag)) for flag in DRC_FLAGS if cfg.inverse_problem.get(flag) is not None}
    out.update(given)
    try:
        P.DynamicRangeOperator(**out)                                              # the operator's own refusals, before any GPU work
    except ValueError as e:
        raise SystemExit(f"-t {DECOMPRESSION}: {e}")
    return out


def warp_params(args, cfg=None, length=16000, sample_rate=16000):
    """The argument rules of -t music_wow_flutter (and of -t music_blind_wow_flutter, whose TRUE curve they build) -> the keyword arguments of `wow_curve`: `components` from every --wow flag (the config's
    `wow` list without one) and `speed_percent` from --speed_pct (the config's `speed_pct`).  A curve for `length` samples is built once
    here so that `wow_curve`'s own refusals come before any GPU work.  Any other task refuses the flags."""
    if args.task not in (WOW_FLUTTER, BLIND_WOW):
        if args.wow is not None or args.speed_pct is not None:
            raise SystemExit(f"--{'wow' if args.wow is not None else 'speed_pct'} belongs to -t {WOW_FLUTTER} and -t {BLIND_WOW}")
        return None
    ip = cfg.inverse_problem if cfg is not None else {}
    if args.wow is not None:
        components = []
        for text in args.wow:
            try:
                c = tuple(float(v) for v in text.split(","))
            except ValueError:
                raise SystemExit(f"--wow {text!r}: RATE_HZ,DEPTH_PCT[,PHASE_DEG]")
            if len(c) not in (2, 3):
                raise SystemExit(f"--wow {text!r}: RATE_HZ,DEPTH_PCT[,PHASE_DEG]")
            components.append(c)
    else:
        components = [tuple(float(v) for v in c) for c in (ip.get("wow") or ())]
    speed = args.speed_pct if args.speed_pct is not None else float(ip.get("speed_pct") or 0.0)
    out = dict(components=tuple(components), speed_percent=float(speed))
    try:
        P.wow_curve(length, sample_rate, **out)
    except ValueError as e:
        raise SystemExit(f"-t {args.task}: {e}")
    return out


def blind_warp_params(args, cfg=None):
    """The argument rules of -t music_blind_wow_flutter -> the keyword arguments `knot_stride`, `max_delay` and `lr` of the
    BlindTimeWarpOperator: each from its --warp_* flag, else from the task's config, else the operator's default.  The operator's own
    refusals (a stride that is no power of two up to 64, max_delay above min(4096, 8 * knot_stride)) come here, before any GPU work.  Any
    other task refuses the flags."""
    flags = dict(knot_stride=args.warp_knot_stride, max_delay=args.warp_max_delay, lr=args.warp_lr)
    if args.task != BLIND_WOW:
        for name, v in flags.items():
            if v is not None:
                raise SystemExit(f"--warp_{name} belongs to -t {BLIND_WOW}")
        return None
    ip = cfg.inverse_problem if cfg is not None else {}
    out = dict(knot_stride=16, max_delay=128.0, lr=0.1)
    for name, v in flags.items():
        if v is None:
            v = ip.get(name)
        if v is not None:
            out[name] = int(v) if name == "knot_stride" else float(v)
    try:
        P.BlindTimeWarpOperator(**out)
    except ValueError as e:
        raise SystemExit(f"-t {BLIND_WOW}: {e}")
    return out


def blind_drc_params(args, cfg=None):
    """The argument rules of -t music_blind_decompression -> dict(operator=the keyword arguments of the BlindDynamicRangeOperator, true=the
    parameters of the synthetic measurement).  The --drc_* flags of music_decompression give the TRUE compressor (--drc_knee_db the knee
    width both sides share), --drc_fit the fitted names and --drc_init_* the start; each falls back to the task's config and then to the
    operator's defaults.  The operator's own refusals come here, before any GPU work.  Any other task refuses --drc_fit and --drc_init_*."""
    init = {flag: getattr(args, f"drc_init_{flag}") for flag in DRC_INIT_FLAGS if getattr(args, f"drc_init_{flag}") is not None}
    if args.task != BLIND_DRC:
        if args.drc_fit is not None:
            raise SystemExit(f"--drc_fit belongs to -t {BLIND_DRC}")
        if init:
            raise SystemExit(f"--drc_init_{next(iter(init))} belongs to -t {BLIND_DRC}")
        return None
    ip = cfg.inverse_problem if cfg is not None else {}
    true = dict(P.BlindDynamicRangeOperator.INIT, threshold_db=-24.0, ratio=4.0, makeup_db=3.0)
    true.update({k: float(v) for k, v in dict(ip.get("true") or {}).items()})
    true.update({flag: getattr(args, f"drc_{flag}") for flag in DRC_INIT_FLAGS if getattr(args, f"drc_{flag}") is not None})
    op_kw = {}
    for name in ("lr", "betas", "adam_eps", "threshold_range", "makeup_range", "time_range_ms"):
        if ip.get(name) is not None:
            v = ip.get(name)
            op_kw[name] = {k: float(x) for k, x in dict(v).items()} if name == "lr" else (float(v) if name == "adam_eps" else tuple(float(x) for x in v))
    knee = args.drc_knee_db if args.drc_knee_db is not None else ip.get("knee_db")
    if knee is not None:
        op_kw["knee_db"] = float(knee)
    fit = args.drc_fit.split(",") if args.drc_fit is not None else ip.get("fit")
    if fit is not None:
        op_kw["fit"] = tuple(str(n).strip() for n in fit)
    start = {k: float(v) for k, v in dict(ip.get("init") or {}).items()}
    start.update(init)
    if start:
        op_kw["init"] = start
    try:
        P.BlindDynamicRangeOperator(**op_kw)._fixed(true, "the measurement's --drc_* parameters")
    except ValueError as e:
        raise SystemExit(f"-t {BLIND_DRC}: {e}")
    return dict(operator=op_kw, true=true)


def separation_stems(args):
    """The argument rules of -t music_source_separation -> K, the number of stems; any other task refuses the separation flags."""
    if args.task != SEPARATION:
        for flag in ("gains", "mixture", "stems"):
            if getattr(args, flag) is not None:
                raise SystemExit(f"--{flag} belongs to -t {SEPARATION}")
        return None
    if args.mixture is not None and args.wav:
        raise SystemExit("--mixture is a real mixture and --wav names the stems of a synthetic one: pass one of them")
    if args.mixture is not None and args.stems is None:
        raise SystemExit("--mixture needs --stems K: the number of stems to restore")
    if args.stems is not None and args.wav and args.stems != len(args.wav):
        raise SystemExit(f"--stems {args.stems} with {len(args.wav)} --wav files: every --wav is one stem")
    K = args.stems if args.stems is not None else (len(args.wav) or 2)
    if not 1 <= K <= 16:
        raise SystemExit(f"{K} stems: a mixture holds 1 .. 16")
    if args.gains is not None and len(args.gains) != K:
        raise SystemExit(f"--gains has {len(args.gains)} values for {K} stems")
    if args.batch != 1:
        raise SystemExit("--batch: one mixture per call, its stems are the batch (--stems)")
    return K


def run_separation(args, cfg, K):
    """-t music_source_separation: K stems from their mixture, MixtureOperator(IdentityOperator) or, with --track_overlap_s, around a track."""
    device = torch.device("cuda")
    pipe_kw = dict(cfg.model.pipe)
    if args.num_inference_steps:
        pipe_kw["num_inference_steps"] = args.num_inference_steps
    sr, length = cfg.data.sample_rate, int(pipe_kw["audio_length_in_s"] * cfg.data.sample_rate)
    whole = args.track_overlap_s is not None
    if args.mixture is not None:
        gt, y = None, load_clips([args.mixture], 1, sr, length, args.seed, whole=whole).to(device)
    elif whole:
        stems = [load_clips(args.wav[k:k + 1], 1, sr, length, args.seed + k, whole=True)[0] for k in range(K)]
        gt = torch.stack([x[:min(len(x) for x in stems)] for x in stems]).to(device)              # the stems end together
    else:
        gt = torch.cat([load_clips(args.wav[k:k + 1], 1, sr, length, args.seed + k) for k in range(K)]).to(device)
    T = (y if gt is None else gt).shape[1]
    inner = P.IdentityOperator(sample_rate=sr)
    noiser = P.get_noiser(**cfg.inverse_problem.noise)
    if getattr(noiser, "additive_sigma", 0.0) > 0:
        inner.noiser = noiser                                                       # drawn inside every guided step too
    layout = P.TrackLayout(T, length, int(round(args.track_overlap_s * sr))) if whole else None
    op = P.MixtureOperator(inner if layout is None else P.TrackOperator(inner, layout), K, args.gains)
    G = op.groups
    if gt is not None:
        y = op.forward(gt)
        y = noiser(y) if inner.noiser is not None else y
    print(f"source separation: {K} stems, gains {args.gains or [1.0] * K}, {T / sr:.2f} s" + (f" as {G} windows per stem" if layout else ""))
    pipe = get_pipeline(cfg.model.name).from_pretrained(args.weights, seed=args.seed).to(device)
    pipe.scheduler = get_scheduler(cfg.name)(operator=op, **dict(cfg.model.scheduler, per_clip_norm=False))
    if args.prompt_embeds:
        pe = torch.from_numpy(np.load(args.prompt_embeds)).float()                  # (K, 512): one prompt per stem
        if pe.shape[0] != K:
            raise SystemExit(f"--prompt_embeds holds {pe.shape[0]} rows, the mixture has {K} stems")
    else:
        pe = torch.nn.functional.normalize(torch.randn(K, 512, generator=torch.Generator().manual_seed(args.seed)), dim=-1)
    pe = pe.repeat_interleave(G, dim=0)                                             # stem-major rows: stem k's windows are contiguous
    gens = [torch.Generator().manual_seed(args.seed + i) for i in range(K * G)]
    if args.init == "measurement":
        init = (y[:, :T] / K).repeat(K, 1)                                          # every stem starts from its share of the mixture
        pipe_kw.update(init_audio=init if layout is None else torch.cat([layout.cut(r) for r in init]), strength=args.strength)
    elif args.strength != 1.0:
        raise SystemExit("--strength needs --init measurement (a cold start runs every step)")
    audio = pipe(prompt_embeds=pe, measurement=y, eta=cfg.scheduler.eta, ip_guidance_rate=cfg.scheduler.ip_guidance_rate, generator=gens,
                 show_progress=args.show_progress, supervised_space=args.supervised_space, **pipe_kw).audios          # (K, T)
    if args.project:
        audio = op.project(torch.from_numpy(audio[:, :T]), y).cpu().numpy()
    out = Path(args.output_dir, cfg.model.name, cfg.data.name, args.config_name, args.task)
    for d in ("wav_input", "wav_recon", "wav_label"):
        os.makedirs(out / d, exist_ok=True)
    scipy.io.wavfile.write(out / "wav_input" / "mixture.wav", sr, y[0].float().cpu().numpy())
    names = [Path(args.wav[k]).stem if k < len(args.wav) else f"stem_{k}" for k in range(K)]
    for k in range(K):
        scipy.io.wavfile.write(out / "wav_recon" / f"{names[k]}.wav", sr, audio[k, :T])
        if gt is not None:
            scipy.io.wavfile.write(out / "wav_label" / f"{names[k]}.wav", sr, gt[k].cpu().numpy())
    line = f"wrote {K} stem(s) to {out}"
    if gt is not None:
        db = ScaleInvariantSDR().score(gt.cpu().numpy(), audio[:, :T])
        line += "; SI-SDR (dB) per stem: " + " ".join(f"{names[k]} {db[k]:.2f}" for k in range(K))
    print(line)


def main(argv=None):
    args = parse_args(argv)
    overrides = [f"data={args.data}", f"model={args.model}"]
    if args.task in ("music_declipping", "music_blind_dereverberation", SEPARATION, SPECTRAL, BLIND_EQ, DECOMPRESSION, WOW_FLUTTER, BLIND_WOW,
                     BLIND_DRC, DECLICK, CODEC):
        overrides.append(f"inverse_problem={args.task}")
    stems = separation_stems(args)
    if args.project and args.task not in ("music_declipping", SEPARATION, DECLICK, CODEC):
        raise SystemExit("--project is the output stage of -t music_declipping, -t music_source_separation, -t music_declicking and "
                         "-t music_codec_restoration")
    cfg = compose(args.config_name, overrides=overrides)
    tf_boxes = spectral_boxes(args, cfg)
    eq_true = equalization_curve(args, cfg)
    drc = compressor_params(args, cfg)
    warp = warp_params(args, cfg, length=int(cfg.model.pipe.audio_length_in_s * cfg.data.sample_rate), sample_rate=cfg.data.sample_rate)
    blind_warp = blind_warp_params(args, cfg)
    blind_drc = blind_drc_params(args, cfg)
    declick = declick_params(args, cfg)
    codec = codec_params(args, cfg)
    if stems is not None:
        if args.model != "musicldm":
            raise SystemExit("this driver feeds MusicLDM's class-embedding conditioning; AudioLDM2 needs its T5 / GPT-2 states (see bench.py --workload)")
        return run_separation(args, cfg, stems)
    if args.model != "musicldm":
        raise SystemExit("this driver feeds MusicLDM's class-embedding conditioning; AudioLDM2 needs its T5 / GPT-2 states (see bench.py --workload)")
    device = torch.device("cuda")
    pipe_kw = dict(cfg.model.pipe)
    if args.num_inference_steps:
        pipe_kw["num_inference_steps"] = args.num_inference_steps
    sr, length = cfg.data.sample_rate, int(pipe_kw["audio_length_in_s"] * cfg.data.sample_rate)
    sched_kw = dict(cfg.model.scheduler)
    layout = None
    if args.track_overlap_s is None:
        gt = load_clips(args.wav, args.batch, sr, length, args.seed).to(device)
        thr = P.threshold_for_sdr(gt, args.clip_sdr_db) if args.task == "music_declipping" else None
        op, scale = build_operator(args.task, cfg, args.mask_type, clip_threshold=thr, tf_boxes=tf_boxes, eq_true=eq_true, drc=drc, warp=warp,
                                   blind_warp=blind_warp, blind_drc=blind_drc, declick=declick, codec=codec, codec_audio=gt)
        B = gt.shape[0]
    else:
        if args.task == "music_generation":
            raise SystemExit("--track_overlap_s restores a recording: pick an inverse problem with -t")
        gt = load_clips(args.wav, 1, sr, length, args.seed, whole=True).to(device)                 # (1, T), T >= one window
        T = gt.shape[1]
        layout = P.TrackLayout(T, length, int(round(args.track_overlap_s * sr)))
        thr = float(P.threshold_for_sdr(gt, args.clip_sdr_db)[0]) if args.task == "music_declipping" else None
        inner, scale = build_operator(args.task, cfg, args.mask_type, audio_length_in_s=P.seconds_for_samples(T, sr), clip_threshold=thr,
                                      tf_boxes=tf_boxes, eq_true=eq_true, drc=drc, warp=warp, blind_warp=blind_warp,
                                      blind_drc=blind_drc, declick=declick, codec=codec, codec_audio=gt[0])
        op = P.TrackOperator(inner, layout)
        B = layout.num_windows
        sched_kw["per_clip_norm"] = False                                          # one loss, norms over all windows
        print(f"track mode: {T / sr:.2f} s as {B} windows of {length / sr:.2f} s, starts (s) {[round(s / sr, 2) for s in layout.starts]}")
    pipe = get_pipeline(cfg.model.name).from_pretrained(args.weights, seed=args.seed).to(device)
    pipe.scheduler = get_scheduler(cfg.name)(operator=op, **sched_kw)
    if args.task == DECLICK:                                                       # clean + clicks (+ noise): the clicks are not part of A
        measurement = op.forward(gt, clicks=synthetic_clicks(op.inner if layout is not None else op, gt, sr))
    else:
        measurement = op.forward(gt)                                               # run.py:290-300: degrade the ground truth once
    if args.prompt_embeds:
        pe = torch.from_numpy(np.load(args.prompt_embeds)).float()
    else:
        pe = torch.nn.functional.normalize(torch.randn(1 if layout else B, 512, generator=torch.Generator().manual_seed(args.seed)), dim=-1)
    if layout is not None and pe.shape[0] == 1:
        pe = pe.repeat(B, 1)                                                       # one prompt for every window of the track
    gens = [torch.Generator().manual_seed(args.seed + i) for i in range(B)]
    if args.init == "measurement":
        init = init_from_measurement(args.task, measurement, gt.shape[1])
        pipe_kw.update(init_audio=init if layout is None else layout.cut(init[:, :gt.shape[1]]), strength=args.strength)
    elif args.strength != 1.0:
        raise SystemExit("--strength needs --init measurement (a cold start runs every step)")
    audio = pipe(prompt_embeds=pe[:B], measurement=measurement, eta=cfg.scheduler.eta, ip_guidance_rate=cfg.scheduler.ip_guidance_rate,
                 generator=gens, show_progress=args.show_progress, supervised_space=args.supervised_space, **pipe_kw).audios
    B, length = gt.shape                                                           # what is written: the clips, or the one track
    if args.project:                                                               # reliable samples kept, clipped ones made consistent
        audio = (op.inner if layout is not None else op).project(torch.from_numpy(audio[:, :length]), measurement).cpu().numpy()
    out = Path(args.output_dir, cfg.model.name, cfg.data.name, args.config_name, args.task)
    for d in ("wav_input", "wav_recon", "wav_label", "mel_recon"):
        os.makedirs(out / d, exist_ok=True)
    to_mel = P.IdentityOperator(sample_rate=sr)                                     # log-mel of the result, like run.py:345-350
    for i in range(B):
        name = Path(args.wav[i]).stem if i < len(args.wav) else f"synthetic_{args.seed + i}"
        scipy.io.wavfile.write(out / "wav_label" / f"{name}.wav", sr, gt[i].cpu().numpy())
        if args.task != "phase_retrieval" and measurement.dim() == 2:
            scipy.io.wavfile.write(out / "wav_input" / f"{name}.wav", sr // scale, measurement[i].float().cpu().numpy())
        scipy.io.wavfile.write(out / "wav_recon" / f"{name}.wav", sr, audio[i])
        mel = to_mel.transform(torch.from_numpy(audio[i:i + 1]).to(device))[0].T      # (frames, 64)
        pipe.save_mel_spectrogram(mel[: length * 100 // sr], out / "mel_recon" / f"{name}.png")
    blind = op.inner if layout is not None else op
    if isinstance(blind, P.DeclickOperator) and blind.last_masked_fraction is not None:
        print(f"click mask: {100.0 * blind.last_masked_fraction:.3f} % of the samples hidden from the loss"
              + (" (--project: meaningful after --supervised_space wav_form only)" if args.project and args.supervised_space != "wav_form" else ""))
    if isinstance(blind, P.BlindDereverberationOperator) and blind.true_ir is not None and blind.ir_estimate is not None:
        est, true = blind.ir_estimate.cpu(), blind.true_ir                         # the synthetic measurement knows its response
        err = torch.linalg.vector_norm(est - true, dim=1) / torch.linalg.vector_norm(true, dim=1)
        print("impulse response estimate, relative error per clip: " + " ".join(f"{e:.3f}" for e in err.tolist()))
    if isinstance(blind, P.BlindEqualizationOperator) and blind.true_curve is not None and blind.eq_estimate is not None:
        est, true = blind.eq_estimate.cpu(), blind.true_curve                      # the synthetic measurement knows its curve
        err = torch.linalg.vector_norm(est - true, dim=1) / torch.linalg.vector_norm(true, dim=1)
        print("equalisation curve estimate, relative error per clip: " + " ".join(f"{e:.3f}" for e in err.tolist()))
    if isinstance(blind, P.BlindTimeWarpOperator) and blind.true_delay is not None and blind.delay_estimate is not None:
        est, true = blind.delay_estimate.cpu(), blind.true_delay                   # the synthetic measurement knows its curve
        true = true - true.mean(dim=1, keepdim=True) if blind.anchor == "mean" else true      # a constant delay is not identified
        err = torch.linalg.vector_norm(est - true, dim=1) / torch.linalg.vector_norm(true, dim=1).clamp_min(1e-30)
        print("delay curve estimate, relative error per clip (mean removed): " + " ".join(f"{e:.3f}" for e in err.tolist()))
    if isinstance(blind, P.BlindDynamicRangeOperator) and blind.true_params is not None and blind.drc_estimate is not None:
        t = blind.true_params                                                      # the synthetic measurement knows its compressor
        print(f"compressor estimate per clip (threshold_db, ratio, makeup_db, attack_ms, release_ms); true {t['threshold_db']:g}, "
              f"{t['ratio']:g}, {t['makeup_db']:g}, {t['attack_ms']:g}, {t['release_ms']:g}: "
              + "; ".join(", ".join(f"{v:.3g}" for v in row) for row in blind.drc_estimate))
    ref = gt.cpu().numpy()
    print(f"wrote {B} clip(s) to {out}; LSD {LogSpectralDistance().score(ref, audio[:, :length]):.4f}  MSE {MeanSquaredError().score(ref, audio[:, :length]):.6f}")


if __name__ == "__main__":
    main()
