"""CPU (gloo): ``gather_rows``, the collective that brings every rank's metric rows to rank 0 in ``evaluate --gpus N``."""
import os
import sys

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rank -> the rows it holds; rank 1 holds nothing
HOLDS = {2: {0: [(1, "b.wav", 1.5), (0, "a.wav", float("nan"))], 1: []},
         3: {0: [(4, "e.wav", 0.25)], 1: [], 2: [(1, "b.wav", 2.0), (2, "c.wav", -1.0), (0, "a.wav", 7.0), (3, "d.wav", 0.0)]}}


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from flowmse_amd.parallel import gather_rows
    out = gather_rows(HOLDS[world][rank])
    if rank == 0:
        q.put([(i, n, repr(v)) for i, n, v in out])
    else:
        assert out is None
    dist.destroy_process_group()


def _run(world, port):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(100)
        assert p.exitcode == 0
    got = q.get(timeout=5)
    want = [(i, n, repr(v)) for r in range(world) for i, n, v in HOLDS[world][r]]
    assert got == want                                       # one flat list, rank order, every row exactly once
    assert sorted(i for i, _, _ in got) == list(range(len(got)))


@pytest.mark.timeout(120)
def test_gather_rows_world2_gloo():
    _run(2, 35500 + os.getpid() % 2000)


@pytest.mark.timeout(120)
def test_gather_rows_world3_one_rank_empty_gloo():
    _run(3, 37500 + os.getpid() % 2000)
