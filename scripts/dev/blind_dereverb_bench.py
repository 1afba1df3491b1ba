#!/usr/bin/env python
"""Measurements that go with blind dereverberation -> profiles/blind_dereverb.json.

    python scripts/dev/blind_dereverb_bench.py ab --parent DIR [--steps 20 --warmup 3 --rounds 2] --out FILE
    python scripts/dev/blind_dereverb_bench.py wgrad [--samples 160000 --taps 5000 --batch 8 --iters 20 --rounds 5] --out FILE
    python scripts/dev/blind_dereverb_bench.py step [--steps 10 --warmup 3 --rounds 3] --out FILE

`ab`: the FIR kernels gained a response stride and the guided-step driver a hook, both on paths every operator runs, so the headline
workload is measured on a build of the parent commit (DIR: a checkout of it with its libraries built) and on this tree, interleaved on
the same device, each `python bench.py --dump-outputs` a fresh process (the procedure of scripts/dev/declip_bench.py `ab`, reused).
Recorded: bit-equality of the dumped latents and losses, every steps/s figure and the parent's own spread.

`wgrad`: the weight-gradient launch next to the dense transpose launch (`fir_clip_bwd`) of the same shape in the same run; both do
batch * taps * Lout fused multiply-adds.  HIP-event windows of `iters` back-to-back launches, the two alternating over `rounds`; recorded:
milliseconds per launch, achieved FLOP/s against the fp32 vector peak, the ratio, and the update launch on its own.

`step`: a blind dereverberation step at the headline shapes (MusicLDM, DPS, batch 8, 10 s clips, 5000 taps) next to a `fixed_ir`
dereverberation step of the same build: steps/s per round, medians, and the operator stage's device milliseconds.

Each subcommand merges its result into the JSON file given with --out."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
from declip_bench import cmd_ab as _parent_ab, merge                               # noqa: E402

PEAK_FP32_VECTOR = 157.3e12          # MI355X datasheet, FLOP/s


def cmd_ab(a):
    """declip_bench's procedure; its result lands under "parent_ab" of --out."""
    _parent_ab(a)


def _window(fn, iters):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def cmd_wgrad(a):
    import torch
    sys.path.insert(0, ROOT)
    from diffmusic_amd import ops
    h_ = ops.load()
    dev = torch.device("cuda")
    B, L, n = a.batch, a.samples, a.taps
    Lout = L + 2 * (n // 2) - n + 1
    g = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(B, L + 32, generator=g)).to(dev)
    dy = torch.randn(B, Lout, generator=g).to(dev)
    h = torch.randn(B, n, generator=g)
    h = (h / h.abs().amax(dim=1, keepdim=True)).to(dev)
    rev = torch.flip(h, dims=[1]).contiguous()
    m, v = torch.zeros_like(h), torch.zeros_like(h)
    part = h_.fir_wgrad(dy, x, L, n)
    legs = {"wgrad": lambda: h_.fir_wgrad(dy, x, L, n), "dense_transpose": lambda: h_.fir_clip_bwd(dy, h, rev, L, L + 32),
            "dense_forward": lambda: h_.fir_clip_fwd(x, h, L), "update": lambda: h_.ir_update(part, h, rev, m, v, 1, 1e-6, 0.9, 0.999, 1e-8)}
    for fn in legs.values():                                 # warm up every shape of the timed windows
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            ms[k].append(round(_window(fn, a.iters), 5))
    med = {k: statistics.median(v) for k, v in ms.items()}
    flop = 2.0 * B * n * Lout
    res = {"batch": B, "samples": L, "taps": n, "Lout": Lout, "segments": int(part.shape[1]), "iters_per_window": a.iters, "rounds": a.rounds,
           "ms_per_launch": ms, "median_ms": med, "fma_flop_per_launch": flop,
           "tflops": {k: round(flop / (med[k] * 1e-3) / 1e12, 3) for k in ("wgrad", "dense_transpose", "dense_forward")},
           "share_of_fp32_vector_peak": {k: round(flop / (med[k] * 1e-3) / PEAK_FP32_VECTOR, 4) for k in ("wgrad", "dense_transpose", "dense_forward")},
           "wgrad_over_dense_transpose_time": round(med["wgrad"] / med["dense_transpose"], 4),
           "partials_mbytes": round(part.numel() * 4 / 1e6, 3)}
    merge(a.out, "wgrad_launch", res)
    print(json.dumps(res))


def cmd_step(a):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from diffmusic_amd import inverse_problem as P, profiling
    dev = torch.device("cuda")
    B, n = a.batch, a.taps
    pipe, _, _, lat, cond, L = bench.build_problem(B, 0, dev, "dps_inpainting")
    clips = torch.stack([bench.synth_clip(k, L) for k in range(B)]).to(dev)
    torch.manual_seed(0)
    ops_ = {"fixed_ir": P.MusicDereverberationOperator(n, 0.99, noiser=P.get_noiser("gaussian", 0.0), fixed_ir=True),
            "blind": P.BlindDereverberationOperator(n, 0.99, noiser=P.get_noiser("gaussian", 0.0))}
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
    blind = ops_["blind"]
    err = torch.linalg.vector_norm(blind.ir_estimate.cpu() - blind.true_ir, dim=1) / torch.linalg.vector_norm(blind.true_ir, dim=1)
    res = {"workload": "MusicLDM + DPS, 10 s clips, mel space, dereverberation", "batch": B, "taps": n, "steps": a.steps, "warmup": a.warmup,
           "steps_per_s": rates, "median_steps_per_s": med, "round_spread_rel": {k: round((max(v) - min(v)) / min(v), 5) for k, v in rates.items()},
           "blind_over_fixed_ir": round(med["blind"] / med["fixed_ir"], 5), "operator_stage_ms": stage,
           "estimate_rel_error_after_last_run": [round(float(e), 4) for e in err]}
    merge(a.out, "blind_step", res)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    out = os.path.join(ROOT, "profiles", "blind_dereverb.json")
    ab = sub.add_parser("ab")
    ab.add_argument("--parent", required=True)
    ab.add_argument("--steps", type=int, default=20)
    ab.add_argument("--warmup", type=int, default=3)
    ab.add_argument("--rounds", type=int, default=2)
    ab.add_argument("--limit", type=float, default=240.0, help="time limit of one bench.py process, seconds")
    ab.add_argument("--out", default=out)
    wg = sub.add_parser("wgrad")
    wg.add_argument("--samples", type=int, default=160000)
    wg.add_argument("--taps", type=int, default=5000)
    wg.add_argument("--batch", type=int, default=8)
    wg.add_argument("--iters", type=int, default=20)
    wg.add_argument("--rounds", type=int, default=5)
    wg.add_argument("--out", default=out)
    st = sub.add_parser("step")
    st.add_argument("--steps", type=int, default=10)
    st.add_argument("--warmup", type=int, default=3)
    st.add_argument("--rounds", type=int, default=3)
    st.add_argument("--batch", type=int, default=8)
    st.add_argument("--taps", type=int, default=5000)
    st.add_argument("--out", default=out)
    a = ap.parse_args()
    {"ab": cmd_ab, "wgrad": cmd_wgrad, "step": cmd_step}[a.cmd](a)


if __name__ == "__main__":
    main()
