#!/usr/bin/env python
"""Measurements that go with blind equalisation -> profiles/blind_eq.json.

    python scripts/dev/blind_eq_bench.py ab --parent DIR [--steps 20 --warmup 3 --rounds 2] --out FILE
    python scripts/dev/blind_eq_bench.py kernel [--batch 8 --length 160000 --iters 200] --out FILE
    python scripts/dev/blind_eq_bench.py step [--steps 20 --warmup 5 --rounds 3 --batch 8] --out FILE

`ab`: the feature adds one kernel file, gives the gain of `tf_gain` a frame stride and moves the Adam step of `ir_update` into a header;
no existing call may change.  The headline workload is measured on a build of the parent commit (DIR: a checkout of it with its
libraries built) and on this tree, interleaved `rounds` times on the same device (the `ab` of scripts/dev/declip_bench.py, unchanged):
dumped latents and losses bit-equal, steps/s within the parent's own spread.

`kernel`: one `tf_wgrad` launch at B = 8, L = 160 000 (628 frames per clip, two forward FFTs each, no halo) next to one `tf_gain` launch of
the same shape (a forward and an inverse FFT per frame, 27 % of them halo) and one `tf_curve` launch, device time from HIP events over
`iters` back-to-back launches; `eq_update` of the 40 partial rows the same way.  The expectation to confirm or refute: tf_wgrad is no
slower than tf_gain.

`step`: a blind step (MusicLDM, DPS, 10 s clips, `BlindEqualizationOperator`, mel space, the estimate live) next to a fixed-curve
`TimeFrequencyMaskOperator` step of the same build holding the same true curve.  The expectation: the masked step plus two
launch-latency kernels.  Recorded: steps/s of every round, the medians and the operator stage's device milliseconds for both.

Each subcommand merges its result into the JSON file given with --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from declip_bench import cmd_ab, merge                                              # noqa: E402


def _timed(fn, iters):
    import torch
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(1000.0 * e0.elapsed_time(e1) / iters, 2)


def cmd_kernel(a):
    import torch
    sys.path.insert(0, ROOT)
    from diffmusic_amd import inverse_problem as P, ops
    from diffmusic_amd.inverse_problem.operator import SpectralFrontend
    B, L = a.batch, a.length
    fe = SpectralFrontend(16000, 1024, 160, 64, "hann")
    h = fe._h.value
    x = 0.3 * torch.randn(B, L, device="cuda")
    dy = 0.01 * torch.randn(B, L, device="cuda")
    curve = torch.from_numpy(P.lowpass_curve(16000, 3000.0, 4))[None].expand(B, -1).contiguous().cuda()
    grid = curve[:, None, :].expand(B, P.tf_frames(L), 513).contiguous()
    part = ops.hip.tf_wgrad(h, dy, x, L)
    g, m, v = curve.clone(), torch.zeros_like(curve), torch.zeros_like(curve)
    res = {"batch": B, "length": L, "frames": P.tf_frames(L), "segments": part.shape[1], "iters": a.iters, "us_per_launch": {
        "tf_gain_per_clip_grids": _timed(lambda: ops.hip.tf_gain(h, x, grid, L, L), a.iters),
        "tf_curve_per_clip": _timed(lambda: ops.hip.tf_curve(h, x, curve, L, L), a.iters),
        "tf_wgrad": _timed(lambda: ops.hip.tf_wgrad(h, dy, x, L), a.iters),
        "eq_update": _timed(lambda: ops.hip.eq_update(part, g, m, v, 1, 0.05, 0.9, 0.999, 1e-8, True), a.iters)}}
    us = res["us_per_launch"]
    res["tf_wgrad_over_tf_gain"] = round(us["tf_wgrad"] / us["tf_gain_per_clip_grids"], 4)
    merge(a.out, "tf_wgrad_launch", res)
    print(json.dumps(res))


def cmd_step(a):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from diffmusic_amd import inverse_problem as P, profiling
    dev = torch.device("cuda")
    B = a.batch
    pipe, _, _, lat, cond, L = bench.build_problem(B, 0, dev, "dps_inpainting")
    clips = torch.stack([bench.synth_clip(k, L) for k in range(B)]).to(dev)
    true = P.lowpass_curve(bench.SR, 3000.0, 4)
    grid = torch.from_numpy(true)[:, None].expand(513, P.tf_frames(L)).contiguous()
    ops_ = {"tf_mask": P.TimeFrequencyMaskOperator(bench.SR, grid, noiser=P.get_noiser("gaussian", 0.0)),
            "blind_eq": P.BlindEqualizationOperator(bench.SR, noiser=P.get_noiser("gaussian", 0.0))}
    meas = {"tf_mask": ops_["tf_mask"].forward(clips), "blind_eq": ops_["blind_eq"].forward(clips, curve=true)}
    assert torch.equal(meas["tf_mask"], meas["blind_eq"])
    ts = pipe.scheduler._timesteps_host

    def run(kind, steps, warm):
        pipe.scheduler.operator = ops_[kind]
        ops_[kind].reset_cache()
        x = lat.clone()
        for t in ts[:warm]:
            x, _ = bench.one_step(pipe, x, t, cond, meas[kind], L)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in ts[warm:warm + steps]:
            x, loss = bench.one_step(pipe, x, t, cond, meas[kind], L)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(loss).all()), (kind, loss)
        return steps / dt

    rates = {k: [] for k in ops_}
    for _ in range(a.rounds):
        for kind in ops_:
            rates[kind].append(round(run(kind, a.steps, a.warmup), 4))
    assert ops_["blind_eq"].k == a.steps + a.warmup
    stage = {}
    for kind in ops_:                                        # device time of the operator stage, from HIP events around it
        profiling.enable(events=True)
        run(kind, a.steps, a.warmup)
        stage[kind] = round(profiling.stage_ms()["operator_mel_loss_fwd_bwd"], 4)
        profiling.enable(events=False)
    med = {k: statistics.median(v) for k, v in rates.items()}
    spread = {k: round((max(v) - min(v)) / min(v), 5) for k, v in rates.items()}
    res = {"workload": "MusicLDM + DPS, 10 s clips, mel space", "batch": B, "steps": a.steps, "warmup": a.warmup, "steps_per_s": rates,
           "median_steps_per_s": med, "round_spread_rel": spread, "blind_eq_over_tf_mask": round(med["blind_eq"] / med["tf_mask"], 5),
           "operator_stage_ms": stage}
    merge(a.out, "blind_eq_step", res)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    out = os.path.join(ROOT, "profiles", "blind_eq.json")
    ab = sub.add_parser("ab")
    ab.add_argument("--parent", required=True)
    ab.add_argument("--steps", type=int, default=20)
    ab.add_argument("--warmup", type=int, default=3)
    ab.add_argument("--rounds", type=int, default=2)
    ab.add_argument("--limit", type=float, default=240.0, help="time limit of one bench.py process, seconds")
    ab.add_argument("--out", default=out)
    kn = sub.add_parser("kernel")
    kn.add_argument("--batch", type=int, default=8)
    kn.add_argument("--length", type=int, default=160000)
    kn.add_argument("--iters", type=int, default=200)
    kn.add_argument("--out", default=out)
    st = sub.add_parser("step")
    st.add_argument("--steps", type=int, default=20)
    st.add_argument("--warmup", type=int, default=5)
    st.add_argument("--rounds", type=int, default=3)
    st.add_argument("--batch", type=int, default=8)
    st.add_argument("--out", default=out)
    a = ap.parse_args()
    {"ab": cmd_ab, "kernel": cmd_kernel, "step": cmd_step}[a.cmd](a)


if __name__ == "__main__":
    main()
