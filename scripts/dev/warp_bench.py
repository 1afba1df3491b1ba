#!/usr/bin/env python
"""Measurements that go with wow and flutter -> profiles/time_warp.json.

    python scripts/dev/warp_bench.py ab --parent DIR [--steps 20 --warmup 3 --rounds 2] --out FILE
    python scripts/dev/warp_bench.py kernel [--batch 8 --length 160000 --iters 200] --out FILE
    python scripts/dev/warp_bench.py step [--steps 20 --warmup 5 --rounds 3 --batch 8] --out FILE

`ab`: the feature adds one kernel file and two ops; no existing call may change.  The headline workload is measured on a build of the
parent commit (DIR: a checkout of it with its libraries built) and on this tree, interleaved `rounds` times on the same device (the `ab`
of scripts/dev/declip_bench.py, unchanged): dumped latents and losses bit-equal, steps/s within the parent's own spread.

`kernel`: one `warp_fwd` and one `warp_bwd` launch at B = 8, L = 160 000 (2501 knots per clip; a 0.5 Hz / 1 % wow plus a 9 Hz / 0.2 %
flutter, shared and per clip) next to one `tf_gain` launch of that shape in the same run, device time from HIP events over `iters`
back-to-back calls.  The bar: neither is slower than `tf_gain`.

`step`: a wow-and-flutter step (MusicLDM, DPS, 10 s clips, `TimeWarpOperator` with that curve, mel space) next to the IdentityOperator step
of the same build, alternating.  The identity rides inside the fused guidance pair; the warped step materialises y = A(wav), runs the same
pair on y and pulls the cotangent back through `warp_bwd`: two more launches.  Recorded: steps/s of every round, the medians, their ratio
(the bar is 0.99) and the operator stage's device milliseconds (HIP events) for both.

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

COMPONENTS = ((0.5, 1.0, 0.0), (9.0, 0.2, 0.0))


def _timed(torch, fn, iters):
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
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from diffmusic_amd import inverse_problem as P, ops
    from diffmusic_amd.inverse_problem.operator import SpectralFrontend
    B, L = a.batch, a.length
    shared = torch.from_numpy(P.wow_curve(L, 16000, COMPONENTS)).cuda()
    per = torch.from_numpy(np.stack([P.wow_curve(L, 16000, ((0.5 + 0.1 * b, 1.0, 20.0 * b), (9.0, 0.2, 0.0))) for b in range(B)])).cuda()
    x = torch.randn(B, L, device="cuda")
    dy = torch.randn(B, L, device="cuda")
    fe = SpectralFrontend(16000, 1024, 160, 64, "hann")
    grid = torch.ones(P.tf_frames(L), 513, device="cuda")
    us = {"warp_fwd": _timed(torch, lambda: ops.hip.warp_fwd(x, shared, L), a.iters),
          "warp_bwd": _timed(torch, lambda: ops.hip.warp_bwd(dy, shared, L, L), a.iters),
          "warp_fwd_per_clip_curves": _timed(torch, lambda: ops.hip.warp_fwd(x, per, L), a.iters),
          "warp_bwd_per_clip_curves": _timed(torch, lambda: ops.hip.warp_bwd(dy, per, L, L), a.iters),
          "tf_gain": _timed(torch, lambda: ops.hip.tf_gain(fe._h.value, x, grid, L, L), a.iters)}
    res = {"batch": B, "length": L, "knots": P.warp_knots(L), "iters": a.iters, "largest_delay_samples": round(float(shared.abs().max()), 2),
           "us_per_call": us, "bar": "neither warp_fwd nor warp_bwd slower than tf_gain",
           "meets_bar": bool(max(us["warp_fwd"], us["warp_bwd"], us["warp_fwd_per_clip_curves"], us["warp_bwd_per_clip_curves"]) <= us["tf_gain"])}
    merge(a.out, "warp_launch", res)
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
    curve = P.wow_curve(L, bench.SR, COMPONENTS)
    ops_ = {"identity": P.IdentityOperator(bench.SR), "warp": P.TimeWarpOperator(bench.SR, delay=curve, noiser=P.get_noiser("gaussian", 0.0))}
    meas = {k: op.forward(clips) for k, op in ops_.items()}
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
    stage = {}
    for kind in ops_:                                        # device time of the operator stage, from HIP events around it
        profiling.enable(events=True)
        run(kind, a.steps, a.warmup)
        stage[kind] = round(profiling.stage_ms()["operator_mel_loss_fwd_bwd"], 4)
        profiling.enable(events=False)
    med = {k: statistics.median(v) for k, v in rates.items()}
    spread = {k: round((max(v) - min(v)) / min(v), 5) for k, v in rates.items()}
    res = {"workload": "MusicLDM + DPS, 10 s clips, mel space", "batch": B, "steps": a.steps, "warmup": a.warmup, "steps_per_s": rates,
           "median_steps_per_s": med, "round_spread_rel": spread, "warp_over_identity": round(med["warp"] / med["identity"], 5),
           "bar": 0.99, "meets_bar": bool(med["warp"] / med["identity"] >= 0.99), "operator_stage_ms": stage,
           "largest_delay_samples": round(float(abs(curve).max()), 2)}
    merge(a.out, "warp_step", res)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    out = os.path.join(ROOT, "profiles", "time_warp.json")
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
