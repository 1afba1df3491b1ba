"""Measures track mode on the GPU (needs one; no fallback): one guided step of an 8-window track next to the plain batch-8 step of the
same build -- configs[1]'s networks and scheduler (MusicLDM + DPS inpainting, 10 s windows), overlap R = 1.28 s, so the track is
8 windows = 71.04 s under one loss.  Both legs are the pipeline's own step (`_unet_eps` + `scheduler.step`) on fixed latents at a
mid-trajectory timestep, timed with device events over windows of at least 0.5 s after a warm-up of every shape, alternated.
Then, in separate passes with stage events on, the operator stage (`operator_mel_loss_fwd_bwd`) of both.

Expectation to confirm or refute: track step = plain step + the operator at 7x the length + two launch-latency kernels.

    python scripts/dev/track_bench.py --out profiles/track_mode.json [--repeats 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/dev/track_bench.py --kernels-only      # the two stitch kernels
    python scripts/dev/track_bench.py --merge-kernel-stats DIR/.../*_kernel_stats.csv --out profiles/track_mode.json"""
import argparse
import csv
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

OVERLAP_S = 1.28


def build(device):
    import bench
    from diffmusic_amd import inverse_problem as P
    from diffmusic_amd.schedulers import get_scheduler
    B = 8
    pipe, op, measurement, latents, cond, L = bench.build_problem(B, 0, device)
    pname, sname, eta, rate, task, _, _ = bench.WORKLOADS["dps_inpainting"]
    plain = pipe.scheduler
    R = int(OVERLAP_S * bench.SR)
    T = L + (B - 1) * (L - R)
    lay = P.TrackLayout(T, L, R)
    assert lay.num_windows == B
    inner = P.MusicInpaintingOperator(P.seconds_for_samples(T, bench.SR), bench.SR, "box", 2, 3, 0.3, 0.1, 1.0, noiser=P.get_noiser("gaussian", 0.0))
    top = P.TrackOperator(inner, lay)
    track = get_scheduler(sname)(operator=top, per_clip_norm=False, **bench.SCHED_CFG)
    track.set_timesteps(bench.N_STEPS, device=device)
    y_track = top.forward(torch.cat([bench.synth_clip(k, L) for k in range(B)])[:T][None].to(device))
    pe = cond["class_labels"][:B]
    c = pipe._prepare_cond(pe, pe, 1, True, device)
    t = plain._timesteps_host[len(plain._timesteps_host) // 2]
    kw = dict(eta=eta, ip_guidance_rate=rate, vae=pipe.vae, vocoder=pipe.vocoder, original_waveform_length=L, supervised_space="mel_spectrogram")

    def step(sched, y):
        eps = pipe._unet_eps(latents, t, c, bench.GUIDANCE_SCALE, True)
        return sched.step(eps, t, latents, measurement=y, **kw).prev_sample

    return (lambda: step(plain, measurement)), (lambda: step(track, y_track)), dict(windows=B, window_len=L, overlap=R, track_len=T, timestep=t)


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters, a.elapsed_time(b)


def stage_pass(fn, iters):
    from diffmusic_amd import profiling
    profiling.enable(events=True)
    for _ in range(iters):
        fn()
    ms = profiling.stage_ms()
    profiling.enable(events=False)
    return {k: round(v, 4) for k, v in ms.items()}


def merge_kernel_stats(path, out):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            if "track_stitch" in r.get("Name", ""):
                rows["fwd" if "fwd" in r["Name"] else "bwd"] = dict(calls=int(r["Calls"]), average_us=round(float(r["AverageNs"]) / 1e3, 3),
                                                                    min_us=round(float(r["MinNs"]) / 1e3, 3), max_us=round(float(r["MaxNs"]) / 1e3, 3))
    with open(out) as fh:
        res = json.loads(fh.read())
    res["stitch_kernels_rocprofv3"] = rows or "not measured"
    with open(out, "w") as fh:
        fh.write(json.dumps(res) + "\n")
    print(json.dumps(res["stitch_kernels_rocprofv3"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true", help="a few track steps and nothing else (run under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--merge-kernel-stats", default=None, help="rocprofv3 *_kernel_stats.csv whose track_stitch rows go into --out")
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out)
    assert torch.cuda.is_available(), "needs a GPU"
    plain, track, meta = build(torch.device("cuda"))
    if args.kernels_only:
        for _ in range(12):
            track()
        torch.cuda.synchronize()
        return
    for fn in (plain, track):                                 # warm-up: every shape of the timed windows
        for _ in range(3):
            fn()
    one_p, _ = window_ms(plain, 2)
    one_t, _ = window_ms(track, 2)
    it_p, it_t = max(2, math.ceil(500.0 / one_p)), max(2, math.ceil(500.0 / one_t))
    p_ms, t_ms, win = [], [], []
    for _ in range(max(2, args.repeats)):                     # alternate the legs so that drift hits both
        a, wa = window_ms(plain, it_p)
        b, wb = window_ms(track, it_t)
        p_ms.append(round(a, 3))
        t_ms.append(round(b, 3))
        win.append(round(min(wa, wb), 1))
    sp, st = stage_pass(plain, 5), stage_pass(track, 5)
    key = "operator_mel_loss_fwd_bwd"
    res = dict(meta, workload="dps_inpainting", plain_step_ms=p_ms, track_step_ms=t_ms, shortest_window_ms=min(win),
               track_minus_plain_ms=round(min(t_ms) - min(p_ms), 3), plain_stages_ms=sp, track_stages_ms=st,
               operator_stage_ms=dict(plain=sp.get(key), track=st.get(key)), stitch_kernels_rocprofv3="not measured")
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
