#!/usr/bin/env python
"""Measurements that go with source separation -> profiles/separation.json.

    python scripts/dev/separation_bench.py ab --parent DIR [--steps 20 --warmup 3 --rounds 2] --out FILE
    python scripts/dev/separation_bench.py step [--steps 20 --warmup 5 --rounds 3 --stems 4] --out FILE

`ab`: the feature adds kernels and two branches on the host; no existing call may change.  The headline workload is measured on a
build of the parent commit (DIR: a checkout of it with its libraries built) and on this tree, interleaved `rounds` times on the same
device (the `ab` of scripts/dev/declip_bench.py, unchanged): dumped latents and losses bit-equal, steps/s within the parent's own spread.

`step`: a K-stem mixture step (MusicLDM, DPS, 10 s clips, `MixtureOperator(IdentityOperator, K)`, mel space) next to a batch-K identity
step of the same build, both under `per_clip_norm=False`.  They differ by the two mix launches and by the fused guidance pair running on
one row instead of K.  Recorded: steps/s of every round, the medians and the operator stage's device milliseconds (HIP events) for both.

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


def cmd_step(a):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from diffmusic_amd import inverse_problem as P, profiling
    dev = torch.device("cuda")
    K = a.stems
    pipe, _, _, lat, cond, L = bench.build_problem(K, 0, dev, "dps_inpainting")
    pipe.scheduler.per_clip_norm = False                     # whole-batch norms on both sides: the mixture's rule, and the fair neighbour
    clips = torch.stack([bench.synth_clip(k, L) for k in range(K)]).to(dev)
    ident = P.IdentityOperator(bench.SR)
    ops_ = {"identity_batch": ident, "mixture": P.MixtureOperator(P.IdentityOperator(bench.SR), K)}
    meas = {k: op.forward(clips) for k, op in ops_.items()}
    assert meas["mixture"].shape == (1, L) and meas["identity_batch"].shape == (K, L)
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
        assert loss.numel() == 1 and bool(torch.isfinite(loss).all()), (kind, loss)
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
    res = {"workload": "MusicLDM + DPS, 10 s clips, mel space, per_clip_norm=False", "stems": K, "steps": a.steps, "warmup": a.warmup,
           "steps_per_s": rates, "median_steps_per_s": med, "round_spread_rel": spread,
           "mixture_over_identity_batch": round(med["mixture"] / med["identity_batch"], 5), "operator_stage_ms": stage}
    merge(a.out, "mixture_step", res)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    out = os.path.join(ROOT, "profiles", "separation.json")
    ab = sub.add_parser("ab")
    ab.add_argument("--parent", required=True)
    ab.add_argument("--steps", type=int, default=20)
    ab.add_argument("--warmup", type=int, default=3)
    ab.add_argument("--rounds", type=int, default=2)
    ab.add_argument("--limit", type=float, default=240.0, help="time limit of one bench.py process, seconds")
    ab.add_argument("--out", default=out)
    st = sub.add_parser("step")
    st.add_argument("--steps", type=int, default=20)
    st.add_argument("--warmup", type=int, default=5)
    st.add_argument("--rounds", type=int, default=3)
    st.add_argument("--stems", type=int, default=4)
    st.add_argument("--out", default=out)
    a = ap.parse_args()
    {"ab": cmd_ab, "step": cmd_step}[a.cmd](a)


if __name__ == "__main__":
    main()
