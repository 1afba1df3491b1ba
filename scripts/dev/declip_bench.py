#!/usr/bin/env python
"""Measurements that go with the declipping operator -> profiles/declip.json.

    python scripts/dev/declip_bench.py ab --parent DIR [--steps 20 --warmup 3 --rounds 2] --out FILE
    python scripts/dev/declip_bench.py step [--steps 20 --warmup 5 --rounds 3 --sdr 3] --out FILE

`ab`: the threshold pointer went into the two fused guidance kernels that every mel-space operator runs, so the headline workload is
measured on a build of the parent commit (DIR: a checkout of it with its libraries built) and on this tree, interleaved `rounds` times
on the same device, each `python bench.py --dump-outputs` a fresh process under its own time limit.  Recorded: whether the latents
and losses of the last timed step are bit-equal, every steps/s figure, the parent's own repeat-to-repeat spread, and the verdict of the
rule "this tree's slower repeat is no more than that spread below the parent's slower repeat".

`step`: a declipping step at the headline shapes (MusicLDM, DPS, batch 8, 10 s clips, thresholds for `--sdr` dB input SDR) next to the
IdentityOperator step of the same build.  Both take the fused pair; they differ by one clamp per loaded sample and one compare per stored
sample.  Recorded: steps/s of every round, the medians and the operator stage's device milliseconds (HIP events) for both.

Each subcommand merges its result into the JSON file given with --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def merge(path, key, value):
    data = {}
    if os.path.exists(path):
        with open(path) as fh:
            data = json.load(fh)
    data[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)
        fh.write("\n")


def bench_once(tree, steps, warmup, dump, limit_s):
    """One `python bench.py` in `tree` as a fresh process; returns its steps/s.  Raises on a non-zero exit or a time-out: nothing more is
    started on the device after a failure."""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline",
           "--no-full-trajectory", "--dump-outputs", dump]
    env = {k: v for k, v in os.environ.items() if k not in ("DMX_LIB_PATH", "PYTHONPATH")}
    r = subprocess.run(cmd, cwd=tree, env=env, capture_output=True, text=True, timeout=limit_s)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["value"])


def cmd_ab(a):
    import numpy as np
    parent = os.path.abspath(a.parent)
    if not os.path.exists(os.path.join(parent, "bench.py")):
        raise SystemExit(f"{parent} holds no bench.py: give a checkout of the parent commit with its libraries built")
    rows, equal = {"parent": [], "tree": []}, []
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(a.rounds):
            for tag, tree in (("parent", parent), ("tree", ROOT)):
                rows[tag].append(bench_once(tree, a.steps, a.warmup, os.path.join(tmp, f"{tag}{r}"), a.limit))
                print(f"round {r} {tag}: {rows[tag][-1]:.4f} steps/s", flush=True)
            same = {}
            for name in ("latents", "loss"):
                p, t = (np.load(os.path.join(tmp, f"{tag}{r}", f"{name}.npy")) for tag in ("parent", "tree"))
                same[name] = bool(p.shape == t.shape and p.tobytes() == t.tobytes())
            equal.append(same)
    spread = max(rows["parent"]) - min(rows["parent"])
    res = {"workload": "bench.py dps_inpainting, batch 8", "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "steps_per_s_parent": rows["parent"], "steps_per_s_tree": rows["tree"], "bit_equal": equal,
           "all_bit_equal": all(v for e in equal for v in e.values()),
           "parent_spread": round(spread, 4), "parent_spread_rel": round(spread / min(rows["parent"]), 5),
           "tree_slower_repeat": min(rows["tree"]), "parent_slower_repeat": min(rows["parent"]),
           "tree_within_parent_spread": bool(min(rows["tree"]) >= min(rows["parent"]) - spread)}
    merge(a.out, "parent_ab", res)
    print(json.dumps(res))
    if not res["all_bit_equal"]:
        raise SystemExit("outputs of the parent build and of this tree differ")


def cmd_step(a):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from diffmusic_amd import inverse_problem as P, profiling
    dev = torch.device("cuda")
    B = a.batch
    pipe, _, _, lat, cond, L = bench.build_problem(B, 0, dev, "dps_inpainting")
    clips = torch.stack([bench.synth_clip(k, L) for k in range(B)])
    thr = P.threshold_for_sdr(clips, a.sdr)
    ops_ = {"identity": P.IdentityOperator(bench.SR), "declipping": P.DeclippingOperator(bench.SR, thr, noiser=P.get_noiser("gaussian", 0.0))}
    meas = {k: op.forward(clips.to(dev)) for k, op in ops_.items()}
    share = float((clips.abs() > torch.from_numpy(thr).float()[:, None]).float().mean())
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
    res = {"workload": "MusicLDM + DPS, 10 s clips, mel space, fused guidance pair", "batch": B, "steps": a.steps, "warmup": a.warmup,
           "input_sdr_db": a.sdr, "clipped_share_of_measurement": round(share, 4), "steps_per_s": rates, "median_steps_per_s": med,
           "round_spread_rel": spread, "declipping_over_identity": round(med["declipping"] / med["identity"], 5),
           "operator_stage_ms": stage}
    merge(a.out, "declipping_step", res)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    ab = sub.add_parser("ab")
    ab.add_argument("--parent", required=True)
    ab.add_argument("--steps", type=int, default=20)
    ab.add_argument("--warmup", type=int, default=3)
    ab.add_argument("--rounds", type=int, default=2)
    ab.add_argument("--limit", type=float, default=240.0, help="time limit of one bench.py process, seconds")
    ab.add_argument("--out", default=os.path.join(ROOT, "profiles", "declip.json"))
    st = sub.add_parser("step")
    st.add_argument("--steps", type=int, default=20)
    st.add_argument("--warmup", type=int, default=5)
    st.add_argument("--rounds", type=int, default=3)
    st.add_argument("--batch", type=int, default=8)
    st.add_argument("--sdr", type=float, default=3.0)
    st.add_argument("--out", default=os.path.join(ROOT, "profiles", "declip.json"))
    a = ap.parse_args()
    {"ab": cmd_ab, "step": cmd_step}[a.cmd](a)


if __name__ == "__main__":
    main()
