#!/usr/bin/env python
"""Measurements that go with codec restoration -> profiles/codec.json.

    python scripts/dev/codec_bench.py ab --parent DIR [--steps 20 --warmup 3 --rounds 3] --out FILE
    python scripts/dev/codec_bench.py kernel [--batch 8 --length 160000 --iters 200] --out FILE
    python scripts/dev/codec_bench.py step [--steps 20 --warmup 5 --rounds 3 --batch 8] --out FILE
    python scripts/dev/codec_bench.py resources --out FILE

`ab`: the feature adds one kernel file, three tables to the front end's one device allocation and three entry points; no existing call may
change.  The headline workload is measured on a build of the parent commit (DIR: a checkout of it with its libraries built) and on this
tree, interleaved `rounds` times on the same device (the `ab` of scripts/dev/declip_bench.py, unchanged; every bench.py process has its own
time limit): dumped latents and losses bit-equal, steps/s within the parent's own spread.

`kernel`: one `mdct_quant` launch at B = 8, L = 160 000 (314 frames per clip, two FFTs each) in each mode -- the quantiser with and without
codes, the pass-through, the projection -- with a shared grid and with per-clip grids, next to one `tf_gain` launch of the same shape (629
frames per clip) in the same process: device time from HIP events over `iters` back-to-back launches.

`step`: a codec step (MusicLDM, DPS, 10 s clips, `CodecOperator` with a fixed grid and a 6 kHz cut-off, mel space) next to the
IdentityOperator step of the same build, alternating.  The identity rides inside the fused guidance pair; the codec step materialises
y = A(wav), runs the same pair on y and applies the pass-through transpose: two more launches.

`resources`: VGPRs, LDS and scratch of the three kernel instances from the compiler's resource report (no GPU needed).

Every GPU step runs under a time limit of its own: `ab` starts each bench.py as a process with `--limit` seconds, and `kernel` and `step`
run themselves as one child process each with `--limit` seconds (a child that fails or runs out of time ends the command; nothing more
is started on the device).

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


def _events(fn, iters):
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
    shared = torch.from_numpy(P.codec_step_grid(L, 16000, -30.0, cutoff_hz=6000.0, tilt_db_per_octave=3.0)).t().contiguous().cuda()
    grids = {"shared_grid": shared, "per_clip_grids": shared[None].expand(B, -1, -1).contiguous()}
    res = {"batch": B, "length": L, "frames": P.mdct_frames(L), "tf_gain_frames": P.tf_frames(L), "iters": a.iters, "us_per_launch": {}}
    for kind, g in grids.items():
        codes = ops.hip.mdct_quant(h, x, g, L, L, want_codes=True)[1]
        res["us_per_launch"][kind] = {
            "quant": _events(lambda: ops.hip.mdct_quant(h, x, g, L, L), a.iters),
            "quant_with_codes": _events(lambda: ops.hip.mdct_quant(h, x, g, L, L, want_codes=True), a.iters),
            "pass": _events(lambda: ops.hip.mdct_quant(h, x, g, L, L, passthrough=True), a.iters),
            "project": _events(lambda: ops.hip.mdct_project(h, x, g, codes, L, L), a.iters)}
    gain = torch.ones(P.tf_frames(L), 513, device="cuda")
    res["us_per_launch"]["tf_gain_shared_grid"] = _events(lambda: ops.hip.tf_gain(h, x, gain, L, L), a.iters)
    res["quant_over_tf_gain"] = round(res["us_per_launch"]["shared_grid"]["quant"] / res["us_per_launch"]["tf_gain_shared_grid"], 4)
    merge(a.out, "mdct_quant_launch", res)
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
    grid = P.codec_step_grid(L, bench.SR, -30.0, cutoff_hz=6000.0, tilt_db_per_octave=3.0)
    ops_ = {"identity": P.IdentityOperator(bench.SR), "codec": P.CodecOperator(bench.SR, grid, noiser=P.get_noiser("gaussian", 0.0))}
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
           "median_steps_per_s": med, "round_spread_rel": spread, "codec_over_identity": round(med["codec"] / med["identity"], 5),
           "operator_stage_ms": stage}
    merge(a.out, "codec_step", res)
    print(json.dumps(res))


def cmd_resources(a):
    sys.path.insert(0, ROOT)
    from diffmusic_amd import build
    src = os.path.join(build.CSRC, "mdct_quant.hip")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(r.stderr[-2000:])
    res, name = {}, None
    modes = {"Li0E": "quant", "Li1E": "pass", "Li2E": "project"}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = next((v for k, v in modes.items() if k in m.group(1)), m.group(1))
            res[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)"), ("waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                res[name][key] = int(m.group(1))
    if not res or any(v.get("scratch_bytes_per_lane") != 0 for v in res.values()):
        raise SystemExit(f"a kernel of mdct_quant.hip uses scratch memory, or no report was found: {res}")
    merge(a.out, "mdct_quant_resources", res)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    out = os.path.join(ROOT, "profiles", "codec.json")
    ab = sub.add_parser("ab")
    ab.add_argument("--parent", required=True)
    ab.add_argument("--steps", type=int, default=20)
    ab.add_argument("--warmup", type=int, default=3)
    ab.add_argument("--rounds", type=int, default=3)
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
    for p, limit in ((kn, 180.0), (st, 600.0)):
        p.add_argument("--limit", type=float, default=limit, help="time limit of the measuring child process, seconds")
        p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.cmd in ("kernel", "step") and not a.child:            # the GPU work happens in a child process under its own time limit
        r = subprocess.run([sys.executable, os.path.abspath(__file__), *sys.argv[1:], "--child"], timeout=a.limit)
        raise SystemExit(r.returncode)
    {"ab": cmd_ab, "kernel": cmd_kernel, "step": cmd_step, "resources": cmd_resources}[a.cmd](a)


if __name__ == "__main__":
    main()
