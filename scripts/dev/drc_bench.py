#!/usr/bin/env python
"""Measurements that go with de-compression -> profiles/drc.json.

    python scripts/dev/drc_bench.py ab --parent DIR [--steps 20 --warmup 3 --rounds 2] --out FILE
    python scripts/dev/drc_bench.py kernel [--batch 8 --length 160000 --iters 200] --out FILE
    python scripts/dev/drc_bench.py step [--steps 20 --warmup 5 --rounds 3 --batch 8] --out FILE

`ab`: the feature adds one kernel file and two ops; no existing call may change.  The headline workload is measured on a build of the
parent commit (DIR: a checkout of it with its libraries built) and on this tree, interleaved `rounds` times on the same device (the `ab`
of scripts/dev/declip_bench.py, unchanged): dumped latents and losses bit-equal, steps/s within the parent's own spread.

`kernel`: one `drc_fwd` and one `drc_bwd` (three launches each) at B = 8, L = 160 000 (H = 2500 blocks per clip) next to one `tf_gain`
launch in the same run, device time from HIP events over `iters` back-to-back calls.  The per-stage split comes from a kernel trace of
this subcommand (`rocprofv3 --kernel-trace --stats -- python scripts/dev/drc_bench.py kernel`): the kernels carry stable names.

`step`: a de-compression step (MusicLDM, DPS, 10 s clips, `DynamicRangeOperator` at its defaults, mel space) next to the IdentityOperator
step of the same build, alternating.  The identity rides inside the fused guidance pair; the de-compression step materialises y = A(wav),
runs the same pair on y and pulls the cotangent back through `drc_bwd`: six more launches.  Recorded: steps/s of every round, the medians,
their ratio (the bar is 0.99) and the operator stage's device milliseconds (HIP events) for both.

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


def _gated(torch, B, L, seed=0):
    """gated noise: about -34 / -6 dBFS in alternating segments of 1000 samples"""
    g = torch.Generator().manual_seed(seed)
    env = torch.where((torch.arange(L) // 1000) % 2 == 0, 0.02, 0.5)
    return (env[None] * torch.randn(B, L, generator=g)).cuda()


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
    import torch
    sys.path.insert(0, ROOT)
    from diffmusic_amd import inverse_problem as P, ops
    from diffmusic_amd.inverse_problem.operator import SpectralFrontend
    B, L = a.batch, a.length
    op = P.DynamicRangeOperator(16000)
    x = _gated(torch, B, L)
    dy = torch.randn(B, L, device="cuda")
    y, state, tape = ops.hip.drc_fwd(x, L, *op.params)
    fe = SpectralFrontend(16000, 1024, 160, 64, "hann")
    grid = torch.ones(P.tf_frames(L), 513, device="cuda")
    res = {"batch": B, "length": L, "blocks": -(-L // 64), "iters": a.iters, "blocks_above_threshold": round(float(((tape & 3) == 2).float().mean()), 4),
           "us_per_call": {"drc_fwd": _timed(torch, lambda: ops.hip.drc_fwd(x, L, *op.params), a.iters),
                           "drc_bwd": _timed(torch, lambda: ops.hip.drc_bwd(dy, x, state, tape, L, *op.params), a.iters),
                           "tf_gain": _timed(torch, lambda: ops.hip.tf_gain(fe._h.value, x, grid, L, L), a.iters)}}
    merge(a.out, "drc_launch", res)
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
    ops_ = {"identity": P.IdentityOperator(bench.SR), "drc": P.DynamicRangeOperator(bench.SR, noiser=P.get_noiser("gaussian", 0.0))}
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
    share = float((torch.from_numpy(P.drc_static_curve(_levels(torch, clips), -24.0, 4.0, 6.0)) > 0).double().mean())
    res = {"workload": "MusicLDM + DPS, 10 s clips, mel space", "batch": B, "steps": a.steps, "warmup": a.warmup, "steps_per_s": rates,
           "median_steps_per_s": med, "round_spread_rel": spread, "drc_over_identity": round(med["drc"] / med["identity"], 5),
           "bar": 0.99, "meets_bar": bool(med["drc"] / med["identity"] >= 0.99), "operator_stage_ms": stage,
           "clean_blocks_with_gain_reduction": round(share, 4)}
    merge(a.out, "drc_step", res)
    print(json.dumps(res))


def _levels(torch, clips):
    B, L = clips.shape
    H = -(-L // 64)
    xb = torch.nn.functional.pad(clips.double().cpu(), (0, H * 64 - L)).reshape(B, H, 64)
    return (10.0 * torch.log10((xb * xb).mean(-1) + 1e-10)).numpy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    out = os.path.join(ROOT, "profiles", "drc.json")
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
