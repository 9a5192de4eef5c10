"""A world of CPU processes over gloo for the tests of fashionern_aaai2024_amd.distributed.  TEST INFRASTRUCTURE."""
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_main(rank, world, port, threads, fn, args):
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(threads)
    from fashionern_aaai2024_amd import distributed as fd
    assert fd.init_from_env("gloo")[:2] == (rank, world) == fd.world_info()
    fn(rank, world, *args)
    dist.barrier()
    dist.destroy_process_group()


def spawn(world: int, fn, *args, threads: int = 2) -> None:
    """Run ``fn(rank, world, *args)`` in `world` fresh processes that form one gloo group (`distributed.init_from_env`); the group is
    taken down behind it.  `fn` is a module-level function of the calling test file: the processes are spawned, so it is pickled."""
    mp.spawn(_rank_main, args=(world, free_port(), threads, fn, args), nprocs=world, join=True)
