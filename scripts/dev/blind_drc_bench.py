#!/usr/bin/env python
"""Measurements that go with blind de-compression -> profiles/blind_drc.json.

    python scripts/dev/blind_drc_bench.py ab --parent DIR [--steps 20 --warmup 3 --rounds 2] --out FILE
    python scripts/dev/blind_drc_bench.py kernel [--batch 8 --length 160000 --iters 200] --out FILE
    python scripts/dev/blind_drc_bench.py step [--steps 20 --warmup 5 --rounds 3 --batch 8] --out FILE
    python scripts/dev/blind_drc_bench.py resources --out FILE

`ab`: the feature templates the kernels of drc.hip on their parameter source, moves their level and curve helpers into a header and adds
one kernel file; no existing call may change.  The headline workload is measured on a build of the parent commit (DIR: a checkout of it
with its libraries built) and on this tree, interleaved `rounds` times on the same device (the `ab` of scripts/dev/declip_bench.py,
unchanged): dumped latents and losses bit-equal, steps/s within the parent's own spread.

`kernel`: single-launch times at B = 8, L = 160 000 in one run: `drc_fwd_p` next to `drc_fwd` and `drc_bwd_p` next to `drc_bwd` (three
launches each; the expectation to confirm or refute: equal within the spread, since the serial chain is untouched), and `drc_pgrad` and
`drc_update` (the expectation: launch latency, H = 2500 blocks per clip).  Device time from HIP events over `iters` back-to-back calls,
three repeats each; the spread is over the repeats.

`step`: a blind step (MusicLDM, DPS, 10 s clips, `BlindDynamicRangeOperator`, mel space, all five parameters live) next to a
fixed-parameter `DynamicRangeOperator` step of the same build, alternating.  The project's bar for an operator's extra launches is a ratio
of 0.99.  Recorded: steps/s of every round, the medians, the round-to-round spread and the operator stage's device milliseconds for both.

`resources`: VGPRs, SGPRs, LDS and scratch of the kernels of drc.hip and drc_fit.hip, from the compiler's resource-usage remarks (the
numbers the code object's metadata carries); needs no device.

Each subcommand merges its result into the JSON file given with --out."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from declip_bench import cmd_ab, merge                                              # noqa: E402
from blind_eq_bench import _timed                                                   # noqa: E402

TRUE = dict(threshold_db=-24.0, ratio=4.0, attack_ms=5.0, release_ms=100.0, makeup_db=3.0)
ALL = ("threshold", "ratio", "makeup", "attack", "release")


def cmd_kernel(a):
    import torch
    sys.path.insert(0, ROOT)
    from diffmusic_amd import inverse_problem as P, ops
    B, L, W = a.batch, a.length, 6.0
    x = 0.3 * torch.randn(B, L, device="cuda")
    dy = 0.01 * torch.randn(B, L, device="cuda")
    fixed = P.DynamicRangeOperator(16000, knee_db=W, **TRUE).params
    T, k, _, aA, aR, mk = fixed
    theta = torch.from_numpy(P.drc_table(T, k, aA, aR, mk, W, B)).cuda()
    y, state, tape = ops.hip.drc_fwd_p(x, L, theta, W)
    dx, work, bq0 = ops.hip.drc_bwd_p(dy, x, state, tape, theta, L, W)
    part = ops.hip.drc_pgrad(state, tape, work, bq0, theta, L, W)
    phi = torch.tensor([[T, k, mk, float(torch.log(torch.tensor(aA))), float(torch.log(torch.tensor(aR)))]] * B, device="cuda")
    m, v, th = torch.zeros_like(phi), torch.zeros_like(phi), theta.clone()
    lo, hi = [-60.0, 0.0, -24.0, -6.2, -6.2], [0.0, 1.0, 24.0, 0.0, 0.0]
    calls = {
        "drc_fwd": lambda: ops.hip.drc_fwd(x, L, *fixed),
        "drc_fwd_p": lambda: ops.hip.drc_fwd_p(x, L, theta, W),
        "drc_bwd": lambda: ops.hip.drc_bwd(dy, x, state, tape, L, *fixed),
        "drc_bwd_p": lambda: ops.hip.drc_bwd_p(dy, x, state, tape, theta, L, W),
        "drc_pgrad": lambda: ops.hip.drc_pgrad(state, tape, work, bq0, theta, L, W),
        "drc_update": lambda: ops.hip.drc_update(part, phi, m, v, th, L, 1, [0.25, 0.01, 0.1, 0.02, 0.02], 0.9, 0.999, 1e-8, W, lo, hi)}
    reps = {name: [] for name in calls}
    for _ in range(3):                                       # interleaved: every repeat visits every call
        for name, fn in calls.items():
            reps[name].append(round(_timed(fn, a.iters), 3))
    us = {name: statistics.median(v) for name, v in reps.items()}
    spread = {name: round((max(v) - min(v)) / min(v), 4) for name, v in reps.items()}
    res = {"batch": B, "length": L, "blocks_per_clip": -(-L // 64), "iters": a.iters, "us_per_call_repeats": reps, "us_per_call": us,
           "repeat_spread_rel": spread, "drc_fwd_p_over_drc_fwd": round(us["drc_fwd_p"] / us["drc_fwd"], 4),
           "drc_bwd_p_over_drc_bwd": round(us["drc_bwd_p"] / us["drc_bwd"], 4)}
    merge(a.out, "drc_table_route_and_fit_launches", res)
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
    ops_ = {"drc": P.DynamicRangeOperator(bench.SR, knee_db=6.0, noiser=P.get_noiser("gaussian", 0.0), **TRUE),
            "blind_drc": P.BlindDynamicRangeOperator(bench.SR, knee_db=6.0, fit=ALL, noiser=P.get_noiser("gaussian", 0.0))}
    meas = {"drc": ops_["drc"].forward(clips), "blind_drc": ops_["blind_drc"].forward(clips, params=TRUE)}
    assert torch.equal(meas["drc"], meas["blind_drc"])
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
    assert ops_["blind_drc"].k == a.steps + a.warmup
    stage = {}
    for kind in ops_:                                        # device time of the operator stage, from HIP events around it
        profiling.enable(events=True)
        run(kind, a.steps, a.warmup)
        stage[kind] = round(profiling.stage_ms()["operator_mel_loss_fwd_bwd"], 4)
        profiling.enable(events=False)
    med = {k: statistics.median(v) for k, v in rates.items()}
    spread = {k: round((max(v) - min(v)) / min(v), 5) for k, v in rates.items()}
    res = {"workload": "MusicLDM + DPS, 10 s clips, mel space", "batch": B, "steps": a.steps, "warmup": a.warmup, "steps_per_s": rates,
           "median_steps_per_s": med, "round_spread_rel": spread, "blind_drc_over_drc": round(med["blind_drc"] / med["drc"], 5),
           "operator_stage_ms": stage}
    merge(a.out, "blind_drc_step", res)
    print(json.dumps(res))


def cmd_resources(a):
    sys.path.insert(0, ROOT)
    from diffmusic_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    res = {}
    for src in ("drc.hip", "drc_fit.hip"):
        r = subprocess.run([hipcc, *build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, src), "-o", os.devnull],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(r.stderr[-2000:])
        name = None
        for line in r.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip() or m.group(1)
                name = re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "").replace("void ", ""))
                res[name] = {}
            for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r" SGPRs: (\d+)"),
                             ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"),
                             ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
                m = re.search(pat, line)
                if m and name:
                    res[name][key] = int(m.group(1))
    merge(a.out, "kernel_resources", res)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    out = os.path.join(ROOT, "profiles", "blind_drc.json")
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
    rs = sub.add_parser("resources")
    rs.add_argument("--out", default=out)
    a = ap.parse_args()
    {"ab": cmd_ab, "kernel": cmd_kernel, "step": cmd_step, "resources": cmd_resources}[a.cmd](a)


if __name__ == "__main__":
    main()
