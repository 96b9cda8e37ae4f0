"""The communicator's calls on host bytes (dfh_comm_allgather, dfh_comm_allreduce_sum, dfh_comm_selfcheck; the host-staged
exchange of csrc/dfh_comm.hip) at the edges of their sizes.  The ranks share the one GPU of the test box through a gloo
callback communicator; worlds 1, 2 and 3.

The checks run inside the ranks (torch.multiprocessing.spawn ends every rank when one of them raises); every wait is
bounded by the process group's timeout.  Every expected value is derived: exact bytes, exact counts, and sums taken in
ascending rank order in fp64."""
import datetime
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PG_TIMEOUT = datetime.timedelta(seconds=120)
# bytes per rank: not multiples of 4 or of 16 (the device receive slots are padded to 16), one beyond a page
GATHER_BYTES = [1, 5, 16, 17, 4099]
REFUSAL = "dfh_comm_allreduce_sum: 1 <= n <= 64 host doubles"


def _payload(rank, nbytes):
    """rank's bytes of an all-gather: differ between ranks and along the message"""
    return ((np.arange(nbytes, dtype=np.int64) * 7 + rank * 31 + 1) % 251).astype(np.uint8)


def _addends(rank, n):
    """rank's n values of an all-reduce: (2^53 + 1) - 2^53 = 0 in fp64 (2^53 + 1 rounds to 2^53) but 2^53 + (1 - 2^53) = 1
    — the sum depends on the order, and the element index rotates which rank holds which addend"""
    base = np.array([2.0 ** 53, 1.0, -2.0 ** 53])
    return base[(rank + np.arange(n)) % 3] * (1.0 + np.arange(n))


def _rank_order_sum(world, n):
    s = np.zeros(n)
    for p in range(world):
        s = s + _addends(p, n)
    return s


def _check_gather(comm, rank, world, nbytes):
    comm.stats(reset=True)
    got = comm.allgather(_payload(rank, nbytes))
    assert got.shape == (world, nbytes)
    for p in range(world):
        assert np.array_equal(got[p], _payload(p, nbytes)), "all-gather of %d bytes: rank %d's slot" % (nbytes, p)
    assert comm.stats() == (nbytes * (world - 1), nbytes * (world - 1), 1), (nbytes, comm.stats())


def _scenario(rank, world, dist, comm, capi):
    comm.selfcheck(30.0)
    for nbytes in GATHER_BYTES:
        _check_gather(comm, rank, world, nbytes)
    # different sizes back to back on one communicator: the device buffers of a call are taken anew from the scratch,
    # which the fourth call outgrows (the scratch starts at 1 MiB) and so replaces
    for nbytes in (5, 4099, 1, 700001, 17):
        _check_gather(comm, rank, world, nbytes)
    for n in (1, 64):
        comm.stats(reset=True)
        got = comm.allreduce_sum(_addends(rank, n))
        want = _rank_order_sum(world, n)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n, got, want)
        assert comm.stats() == (8 * n * (world - 1), 8 * n * (world - 1), 1), (n, comm.stats())
        every = [None] * world
        dist.all_gather_object(every, got.tobytes())
        assert len(set(every)) == 1, "the all-reduce of %d values differs between ranks" % n
    if world == 3:  # the order matters in what was summed: the first element is (2^53 + 1) - 2^53
        assert _rank_order_sum(3, 1)[0] == 0.0 and 2.0 ** 53 + (1.0 - 2.0 ** 53) == 1.0
    for n in (0, 65):
        comm.stats(reset=True)
        with pytest.raises(capi.DfhError, match=REFUSAL):
            comm.allreduce_sum(np.zeros(n))
        assert comm.stats() == (0, 0, 0)
    comm.selfcheck(30.0)


def _spawned(rank, world, port):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=PG_TIMEOUT)
    from difacto_amd import capi
    ctx = capi.Context(0)

    def exchange(send, sb, recv, rb):
        out = torch.empty(sum(rb), dtype=torch.uint8)
        dist.all_to_all_single(out, torch.from_numpy(np.array(send, copy=True)), output_split_sizes=rb, input_split_sizes=sb)
        recv[:] = out.numpy()

    comm = capi.Comm.callback(ctx, rank, world, exchange)
    _scenario(rank, world, dist, comm, capi)
    comm.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2, 3])
def test_host_bytes_over_the_communicator(world):
    import torch.multiprocessing as mp
    port = 29300 + (os.getpid() % 90) + world
    # join: a rank that raises ends the others, so none of them is left waiting in a collective
    mp.spawn(_spawned, args=(world, port), nprocs=world, join=True)
