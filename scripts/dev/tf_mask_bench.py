#!/usr/bin/env python
"""Measurements that go with time-frequency masking -> profiles/tf_mask.json.

    python scripts/dev/tf_mask_bench.py ab --parent DIR [--steps 20 --warmup 3 --rounds 2] --out FILE
    python scripts/dev/tf_mask_bench.py kernel [--batch 8 --length 160000 --iters 200] --out FILE
    python scripts/dev/tf_mask_bench.py step [--steps 20 --warmup 5 --rounds 3 --batch 8] --out FILE

`ab`: the feature adds one kernel file and moves the FFT helpers of the fused STFT-mel kernels into a header; no existing call may
change.  The headline workload is measured on a build of the parent commit (DIR: a checkout of it with its libraries built) and on this
tree, interleaved `rounds` times on the same device (the `ab` of scripts/dev/declip_bench.py, unchanged): dumped latents and losses
bit-equal, steps/s within the parent's own spread.

`kernel`: one `tf_gain` launch at B = 8, L = 160 000 (626 + 3 frames per clip, two FFTs each), device time from HIP events over `iters`
back-to-back launches, with a shared grid and with per-clip grids.

`step`: a masked step (MusicLDM, DPS, 10 s clips, `TimeFrequencyMaskOperator` with a band-stop box and a spectral hole, mel space) next to
the IdentityOperator step of the same build.  The identity rides inside the fused guidance pair; the masked step materialises y = A(wav),
runs the same pair on y and applies A again: two more launches.  Recorded: steps/s of every round, the medians and the operator stage's
device milliseconds (HIP events) for both.

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


def _grid(P, L, sr):
    dur = L / sr
    return P.tf_gain_grid(L, sr, [(2000.0, 3000.0, None, None, 0.0), (500.0, 1500.0, 0.4 * dur, 0.6 * dur, 0.0)])


def cmd_kernel(a):
    import torch
    sys.path.insert(0, ROOT)
    from diffmusic_amd import inverse_problem as P, ops
    from diffmusic_amd.inverse_problem.operator import SpectralFrontend
    B, L = a.batch, a.length
    fe = SpectralFrontend(16000, 1024, 160, 64, "hann")
    x = 0.3 * torch.randn(B, L, device="cuda")
    shared = torch.from_numpy(_grid(P, L, 16000)).t().contiguous().cuda()
    grids = {"shared_grid": shared, "per_clip_grids": shared[None].expand(B, -1, -1).contiguous()}
    res = {"batch": B, "length": L, "frames": P.tf_frames(L), "iters": a.iters, "us_per_launch": {}}
    for kind, g in grids.items():
        for _ in range(10):
            ops.hip.tf_gain(fe._h.value, x, g, L, L)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            ops.hip.tf_gain(fe._h.value, x, g, L, L)
        e1.record()
        torch.cuda.synchronize()
        res["us_per_launch"][kind] = round(1000.0 * e0.elapsed_time(e1) / a.iters, 2)
    merge(a.out, "tf_gain_launch", res)
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
    ops_ = {"identity": P.IdentityOperator(bench.SR),
            "tf_mask": P.TimeFrequencyMaskOperator(bench.SR, _grid(P, L, bench.SR), noiser=P.get_noiser("gaussian", 0.0))}
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
           "median_steps_per_s": med, "round_spread_rel": spread, "tf_mask_over_identity": round(med["tf_mask"] / med["identity"], 5),
           "operator_stage_ms": stage}
    merge(a.out, "tf_mask_step", res)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    out = os.path.join(ROOT, "profiles", "tf_mask.json")
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
