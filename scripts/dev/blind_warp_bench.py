#!/usr/bin/env python
"""Measurements that go with blind wow and flutter -> profiles/blind_warp.json.

    python scripts/dev/blind_warp_bench.py ab --parent DIR [--steps 20 --warmup 3 --rounds 2] --out FILE
    python scripts/dev/blind_warp_bench.py kernel [--batch 8 --length 160000 --knot_stride 16 --iters 200] --out FILE
    python scripts/dev/blind_warp_bench.py step [--steps 20 --warmup 5 --rounds 3 --batch 8] --out FILE

`ab`: the feature adds one kernel file and moves the position helpers of warp.hip into a header; no existing call may change.  The
headline workload is measured on a build of the parent commit (DIR: a checkout of it with its libraries built) and on this tree,
interleaved `rounds` times on the same device (the `ab` of scripts/dev/declip_bench.py, unchanged): dumped latents and losses bit-equal,
steps/s within the parent's own spread.

`kernel`: one `warp_wgrad` launch and one `warp_update` launch at B = 8, L = 160 000, knot stride 16, next to one `warp_bwd` and one
`warp_fwd` launch of the same shape and curve, device time from HIP events over `iters` back-to-back launches.  `warp_wgrad` evaluates one
knot pair per sample where `warp_bwd` evaluates about 19 over the same bytes; the expectation to confirm or refute: it is no slower.

`step`: a blind step (MusicLDM, DPS, 10 s clips, `BlindTimeWarpOperator`, mel space, the estimate live) next to a fixed-curve
`TimeWarpOperator` step of the same build holding the true curve, alternating.  The expectation: the fixed-curve step plus two
launch-latency kernels; the project's bar for an operator's extra launches is a ratio of 0.99.  Recorded: steps/s of every round, the
medians, the round-to-round spread and the operator stage's device milliseconds for both.

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
from blind_eq_bench import _timed                                                   # noqa: E402

WOW = ((0.5, 1.0, 0.0), (9.0, 0.2, 0.0))


def cmd_kernel(a):
    import torch
    sys.path.insert(0, ROOT)
    from diffmusic_amd import inverse_problem as P, ops
    B, L, S = a.batch, a.length, a.knot_stride
    x = 0.3 * torch.randn(B, L, device="cuda")
    dy = 0.01 * torch.randn(B, L, device="cuda")
    fine = torch.from_numpy(P.wow_curve(L, 16000, WOW))[None].expand(B, -1).contiguous().cuda()
    n = P.warp_coarse_knots(L, S)
    c = torch.zeros(B, n, device="cuda")
    m, v, d = torch.zeros_like(c), torch.zeros_like(c), fine.clone()
    part = ops.hip.warp_wgrad(dy, x, fine, L)
    M = min(4096.0, 8.0 * S)
    res = {"batch": B, "length": L, "knot_stride": S, "fine_knots": fine.shape[1], "coarse_knots": n, "iters": a.iters, "us_per_launch": {
        "warp_fwd": _timed(lambda: ops.hip.warp_fwd(x, fine, L), a.iters),
        "warp_bwd": _timed(lambda: ops.hip.warp_bwd(dy, fine, L, L), a.iters),
        "warp_wgrad": _timed(lambda: ops.hip.warp_wgrad(dy, x, fine, L), a.iters),
        "warp_update": _timed(lambda: ops.hip.warp_update(part, c, m, v, d, L, S, 1, 0.1, 0.9, 0.999, 1e-8, M, True), a.iters)}}
    us = res["us_per_launch"]
    res["warp_wgrad_over_warp_bwd"] = round(us["warp_wgrad"] / us["warp_bwd"], 4)
    merge(a.out, "warp_wgrad_launch", res)
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
    true = P.wow_curve(L, bench.SR, WOW)
    ops_ = {"warp": P.TimeWarpOperator(bench.SR, delay=true, noiser=P.get_noiser("gaussian", 0.0)),
            "blind_warp": P.BlindTimeWarpOperator(bench.SR, noiser=P.get_noiser("gaussian", 0.0))}
    meas = {"warp": ops_["warp"].forward(clips), "blind_warp": ops_["blind_warp"].forward(clips, delay=true)}
    assert torch.equal(meas["warp"], meas["blind_warp"])
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
    assert ops_["blind_warp"].k == a.steps + a.warmup
    stage = {}
    for kind in ops_:                                        # device time of the operator stage, from HIP events around it
        profiling.enable(events=True)
        run(kind, a.steps, a.warmup)
        stage[kind] = round(profiling.stage_ms()["operator_mel_loss_fwd_bwd"], 4)
        profiling.enable(events=False)
    med = {k: statistics.median(v) for k, v in rates.items()}
    spread = {k: round((max(v) - min(v)) / min(v), 5) for k, v in rates.items()}
    res = {"workload": "MusicLDM + DPS, 10 s clips, mel space", "batch": B, "steps": a.steps, "warmup": a.warmup, "steps_per_s": rates,
           "median_steps_per_s": med, "round_spread_rel": spread, "blind_warp_over_warp": round(med["blind_warp"] / med["warp"], 5),
           "operator_stage_ms": stage}
    merge(a.out, "blind_warp_step", res)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    out = os.path.join(ROOT, "profiles", "blind_warp.json")
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
    kn.add_argument("--knot_stride", type=int, default=16)
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
