#!/usr/bin/env python
"""Cost of the measurement noise inside the guided step on the flagship workload.

bench.py has no sigma switch.  This takes its problem (`bench.build_problem`, dps_inpainting, the workload's batch), swaps in an
operator built with the same arguments and `GaussianNoise(sigma, stream="clip")`, and times the same 20 warmed guided steps
(U-Net + `scheduler.step`, plain loop) between device synchronises, alternating sigma = 0 and sigma > 0:

    python scripts/dev/noise_overhead.py [--sigma 0.05] [--steps 20] [--rounds 3] [--batch 8]

Prints one JSON line: steps/s of every round and the medians."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import bench                                                                        # noqa: E402
from diffmusic_amd import inverse_problem as P                                      # noqa: E402


def timed(pipe, op, lat, cond, meas, L, steps, warm):
    pipe.scheduler.operator = op
    ts = pipe.scheduler._timesteps_host
    x = lat.clone()
    for t in ts[:warm]:
        x, _ = bench.one_step(pipe, x, t, cond, meas, L)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in ts[warm:warm + steps]:
        x, loss = bench.one_step(pipe, x, t, cond, meas, L)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert bool(torch.isfinite(loss).all())
    return steps / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=bench.WORKLOADS["dps_inpainting"][5])
    a = ap.parse_args()
    dev = torch.device("cuda")
    pipe, op0, meas, lat, cond, L = bench.build_problem(a.batch, 0, dev, "dps_inpainting")
    op1 = P.MusicInpaintingOperator(bench.SECONDS, bench.SR, "box", 2, 3, 0.3, 0.1, 1.0, noiser=P.get_noiser("gaussian", a.sigma, stream="clip"))
    quiet, noisy = [], []
    for _ in range(a.rounds):
        quiet.append(timed(pipe, op0, lat, cond, meas, L, a.steps, a.warmup))
        noisy.append(timed(pipe, op1, lat, cond, meas, L, a.steps, a.warmup))
    q, n = statistics.median(quiet), statistics.median(noisy)
    print(json.dumps({"workload": "dps_inpainting", "batch": a.batch, "steps": a.steps, "sigma": a.sigma, "stream": "clip",
                      "steps_per_s_sigma0": [round(v, 3) for v in quiet], "steps_per_s_noisy": [round(v, 3) for v in noisy],
                      "median_sigma0": round(q, 3), "median_noisy": round(n, 3), "noisy_over_sigma0": round(n / q, 4)}))


if __name__ == "__main__":
    main()
