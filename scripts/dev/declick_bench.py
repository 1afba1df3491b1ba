#!/usr/bin/env python
"""Measurements that go with declicking -> profiles/declick.json.

    python scripts/dev/declick_bench.py ab --parent DIR [--steps 20 --warmup 3 --rounds 2] --out FILE
    python scripts/dev/declick_bench.py kernel [--batch 8 --length 160000 --iters 200] --out FILE
    python scripts/dev/declick_bench.py step [--steps 20 --warmup 5 --rounds 3 --batch 8] --out FILE

`ab`: the feature adds one kernel file and four ops; no existing call may change.  The headline workload is measured on a build of the
parent commit (DIR: a checkout of it with its libraries built) and on this tree, interleaved `rounds` times on the same device (the `ab`
of scripts/dev/declip_bench.py, unchanged): dumped latents and losses bit-equal, steps/s within the parent's own spread.

`kernel`: one `click_detect`, one `click_mask`, one `mask_rows` and one `declick_blend` launch at B = 8, L = 160 000 (157 frames per clip;
the bench's synthetic clips plus 20 clicks per second) next to one `tf_gain` launch of that shape in the same run, device time from HIP
events over `iters` back-to-back calls.  No bar: the detector and the dilation run once per trajectory, `mask_rows` twice per step.

`step`: a declick step (MusicLDM, DPS, 10 s clips, `DeclickOperator` with auto-detection, mel space) next to the IdentityOperator step of
the same build, alternating.  The identity rides inside the fused guidance pair; the declick step materialises y = m * wav, runs the same
pair on y and masks the cotangent: two more launches.  Recorded: steps/s of every round, the medians, their ratio (the bar for a
materialised operator is 0.99), the round-to-round spread and the masked fraction.

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
from warp_bench import _timed                                                       # noqa: E402

CLICKS_PER_S, CLICK_AMP = 20.0, (0.3, 0.6)


def _measurement(torch, bench, P, B, L, dev):
    clips = torch.stack([bench.synth_clip(k, L) for k in range(B)]).to(dev)
    clicks = P.click_train(L, bench.SR, CLICKS_PER_S, amplitude=CLICK_AMP, max_width=3, seed=0, batch=B)
    return clips, clicks


def cmd_kernel(a):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from diffmusic_amd import inverse_problem as P, ops
    from diffmusic_amd.inverse_problem.operator import SpectralFrontend
    B, L = a.batch, a.length
    clips, clicks = _measurement(torch, bench, P, B, L, "cuda")
    y = clips + clicks.cuda()
    x = torch.randn(B, L, device="cuda")
    flags = ops.hip.click_detect(y, L, 5.0, 1e-5)[3]
    mask, masked = ops.hip.click_mask(flags, 3)
    fe = SpectralFrontend(16000, 1024, 160, 64, "hann")
    grid = torch.ones(P.tf_frames(L), 513, device="cuda")
    us = {"click_detect": _timed(torch, lambda: ops.hip.click_detect(y, L, 5.0, 1e-5), a.iters),
          "click_mask": _timed(torch, lambda: ops.hip.click_mask(flags, 3), a.iters),
          "click_mask_guard64": _timed(torch, lambda: ops.hip.click_mask(flags, 64), a.iters),
          "mask_rows": _timed(torch, lambda: ops.hip.mask_rows(x, mask, L, L), a.iters),
          "declick_blend_fade16": _timed(torch, lambda: ops.hip.declick_blend(x, y, mask, L, 16), a.iters),
          "tf_gain": _timed(torch, lambda: ops.hip.tf_gain(fe._h.value, x, grid, L, L), a.iters)}
    res = {"batch": B, "length": L, "frames": -(-L // 1024), "iters": a.iters, "masked_fraction": round(float(masked.sum()) / (B * L), 5),
           "us_per_call": us, "note": "each time includes the allocation of the op's outputs; no bar (detector and dilation run once per "
           "trajectory, mask_rows twice per step)"}
    merge(a.out, "declick_launch", res)
    print(json.dumps(res))


def cmd_step(a):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from diffmusic_amd import inverse_problem as P
    dev = torch.device("cuda")
    B = a.batch
    pipe, _, _, lat, cond, L = bench.build_problem(B, 0, dev, "dps_inpainting")
    clips, clicks = _measurement(torch, bench, P, B, L, dev)
    ops_ = {"identity": P.IdentityOperator(bench.SR), "declick": P.DeclickOperator(bench.SR, noiser=P.get_noiser("gaussian", 0.0))}
    meas = {"identity": ops_["identity"].forward(clips), "declick": ops_["declick"].forward(clips, clicks=clicks)}
    ts = pipe.scheduler._timesteps_host

    def run(kind, steps, warm):
        pipe.scheduler.operator = ops_[kind]
        ops_[kind].reset_cache()
        x = lat.clone()
        for t in ts[:warm]:                                  # the detection happens in the first warm-up step, as in a trajectory
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
    med = {k: statistics.median(v) for k, v in rates.items()}
    spread = {k: round((max(v) - min(v)) / min(v), 5) for k, v in rates.items()}
    res = {"workload": "MusicLDM + DPS, 10 s clips, mel space", "batch": B, "steps": a.steps, "warmup": a.warmup, "steps_per_s": rates,
           "median_steps_per_s": med, "round_spread_rel": spread, "declick_over_identity": round(med["declick"] / med["identity"], 5),
           "bar": 0.99, "meets_bar": bool(med["declick"] / med["identity"] >= 0.99),
           "masked_fraction": round(ops_["declick"].last_masked_fraction, 5), "clicks_per_s": CLICKS_PER_S}
    merge(a.out, "declick_step", res)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    out = os.path.join(ROOT, "profiles", "declick.json")
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
