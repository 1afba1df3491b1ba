"""-m gpu: a warm-started call sharded over two rank processes on one GPU (the pattern of tests/test_gpu_multirank.py with a worker of
its own): the clip's init rows are selected first and then encoded, the draws are per clip, and the gathered result is that of the
unsharded call."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(n_clips, out):
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "warm_start_multirank_worker.py"), str(n_clips), out],
                                      env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-1500:] for l in logs)
    return [np.load(out.replace(".npy", f"_rank{rank}.npy")) for rank in range(2)]


def _problem(n_clips):
    from tests.multirank_worker import gens
    from tests.warm_start_multirank_worker import warm_problem
    pipe, kw = warm_problem(n_clips)
    return pipe, kw, gens


def test_sharded_warm_start_equals_the_ranks_clips_run_alone(tmp_path):
    """Rank r's clips (r, r + 2, ...) run without torch.distributed in the same batch composition: bit-equal, on every rank (the contract
    tests/test_gpu_multirank.py holds for the cold path)."""
    n_clips = 5
    got = _run_ranks(n_clips, str(tmp_path / "warm.npy"))
    pipe, kw, gens = _problem(n_clips)
    ref = np.zeros_like(got[0])
    for rank in range(2):
        sel = list(range(rank, n_clips, 2))
        kws = dict(kw, prompt_embeds=kw["prompt_embeds"][sel], measurement=kw["measurement"][sel].contiguous(), init_mel=kw["init_mel"][sel])
        ref[sel] = pipe(generator=[gens(n_clips)[k] for k in sel], **kws).audios.cpu().numpy()
    assert np.isfinite(ref).all() and float(np.abs(ref).max()) > 1e-3
    for rank in range(2):
        assert np.array_equal(got[rank], ref), (rank, float(np.abs(got[rank] - ref).max()))


def test_sharded_warm_start_equals_the_unsharded_call(tmp_path):
    """`shard=True` at world size 2 against ONE call on all clips, bit for bit, as the issue states the check."""
    n_clips = 5
    got = _run_ranks(n_clips, str(tmp_path / "warm.npy"))
    pipe, kw, gens = _problem(n_clips)
    full = pipe(generator=gens(n_clips), **kw).audios.cpu().numpy()
    d = float(np.abs(got[0] - full).max())
    rel = float(np.linalg.norm((got[0] - full).astype(np.float64)) / np.linalg.norm(full.astype(np.float64)))
    print(f"sharded warm start over 2 ranks vs one batch of {n_clips}: max |diff| {d:.3e}, rel-L2 {rel:.3e}")
    assert np.array_equal(got[0], got[1])
    assert np.array_equal(got[0], full)
