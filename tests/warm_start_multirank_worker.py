"""Rank process of tests/test_gpu_warm_start_shard.py (not a test module): the rank process of tests/multirank_worker.py with a warm
start -- every rank joins a gloo group on cuda:0 of a 1-GPU box and runs `Pipeline.__call__(shard=True, init_mel=..., strength=0.5)`
on the small nets; each rank saves the gathered latents of all clips.

    RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/warm_start_multirank_worker.py <n_clips> <out.npy>"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def warm_problem(n_clips):
    """`problem()` of tests/multirank_worker.py plus the init mel and the warm-start keywords (latents out)."""
    from tests.multirank_worker import problem
    pipe, kw = problem(n_clips)
    mel = 2.0 * torch.randn(n_clips, 40, 64, generator=torch.Generator().manual_seed(57)) - 4.0
    return pipe, dict(kw, init_mel=mel, strength=0.5, output_type="latent")


def main():
    n_clips, out_path = int(sys.argv[1]), sys.argv[2]
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    try:
        from tests.multirank_worker import gens
        pipe, kw = warm_problem(n_clips)
        out = pipe(generator=gens(n_clips), shard=True, **kw).audios
        assert out.shape[0] == n_clips and len(pipe.last_losses) == 2, (out.shape, len(pipe.last_losses))
        np.save(out_path.replace(".npy", f"_rank{rank}.npy"), out.cpu().numpy())
        dist.barrier()
    finally:
        dist.destroy_process_group()
    print(f"[worker] rank {rank} done", flush=True)


if __name__ == "__main__":
    main()
