"""Rank process of tests/test_gpu_noise.py::test_clip_stream_two_ranks_bit_equal_to_single_rank (not a test module): the sharding
rehearsal of tests/multirank_worker.py -- same pipeline, clips, conditioning and launch -- with measurement noise inside every guided
step on the per-clip stream (`GaussianNoise(SIGMA, stream="clip")`).

    RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/noise_multirank_worker.py <n_clips> <out.npy> [gloo|nccl]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import multirank_worker as W                                            # noqa: E402

SIGMA = 0.05
gens = W.gens
_quiet_problem = W.problem


def problem(n_clips):
    """The rehearsal's problem (its measurement is built noiseless) with the noisy step switched on."""
    from diffmusic_amd import inverse_problem as P
    pipe, kw = _quiet_problem(n_clips)
    pipe.scheduler.operator.noiser = P.GaussianNoise(SIGMA, stream="clip")
    return pipe, kw


if __name__ == "__main__":
    W.problem = problem
    W.main()
