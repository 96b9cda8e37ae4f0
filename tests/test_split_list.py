"""CPU: the capacity of the split list (dfh_batch_create: split_cap = 2 * (N / 1024) + 16 entries for a batch object of N
pairs) bounds what a training step can list, whatever the minibatch.

A step lists ceil(len / 1024) entries for every segment with len > 4096.  For such a segment
ceil(len / 1024) <= len / 1024 + 1 < len / 1024 + len / 4096 = 1.25 * len / 1024, so the sum over ANY partition of N pairs is
below 1.25 * N / 1024 <= 1.25 * (N // 1024 + 1) <= 2 * (N // 1024) + 16.  lookup_split's clamp can therefore only fire if the
list is not emptied between steps; the GPU tests (tests/test_gpu_parity.py) check the count after every step.
"""
import numpy as np
import pytest

from split_testlib import HOT_SPLIT, HOT_SPLIT_MIN, split_cap, split_entries_expected


def _worst_partition(N):
    """the partition of N that lists the most entries: as many segments of HOT_SPLIT_MIN + 1 as fit (5 entries per 4 097
    pairs, 1.22 per 1 024 — every longer segment lists fewer per pair), the rest in one more segment"""
    m = N // (HOT_SPLIT_MIN + 1)
    return [HOT_SPLIT_MIN + 1] * m + ([N - m * (HOT_SPLIT_MIN + 1)] if N % (HOT_SPLIT_MIN + 1) else [])


@pytest.mark.parametrize("N", [0, 1, 1023, 1024, 4096, 4097, 4098, 5120, 8193, 8194, 16388, 40970, 65536, 390000, 780000,
                               4097 * 1000, (1 << 24) + 5])
def test_worst_partition_fits(N):
    parts = _worst_partition(N)
    assert sum(parts) == N
    assert split_entries_expected(parts) <= split_cap(N)
    # the whole of N in one segment, and one pair short of the next part
    assert split_entries_expected([N]) <= split_cap(N)
    # a batch object may hold FEWER pairs than it was created for, never more
    assert split_entries_expected(parts) <= split_cap(N + 12345)


def test_boundaries_of_the_cut():
    assert split_entries_expected([HOT_SPLIT_MIN]) == 0            # stays whole in the hot role
    assert split_entries_expected([HOT_SPLIT_MIN + 1]) == 5        # five parts, the last of one occurrence
    assert split_entries_expected([5 * HOT_SPLIT]) == 5
    assert split_entries_expected([5 * HOT_SPLIT + 1]) == 6
    assert split_entries_expected([8192, 9, 1, 1, 4096, 4097]) == 8 + 5


def test_random_partitions_fit():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        N = int(rng.integers(1, 1 << 20))
        # segments drawn around the cut, where an entry costs the fewest pairs, until N is used up
        lens, left = [], N
        while left > 0:
            kind = rng.integers(0, 4)
            if kind == 0:
                n = HOT_SPLIT_MIN + 1 + int(rng.integers(0, 3))
            elif kind == 1:
                n = int(rng.integers(1, 6)) * HOT_SPLIT + 1 + HOT_SPLIT_MIN
            elif kind == 2:
                n = int(rng.integers(1, 4 * HOT_SPLIT_MIN))
            else:
                n = int(rng.integers(1, 40))
            n = min(n, left)
            lens.append(n)
            left -= n
        got = split_entries_expected(lens)
        assert got <= split_cap(N), (N, got, split_cap(N))
        assert got <= 1.25 * N / HOT_SPLIT


def test_small_batches_list_nothing():
    """below 4 097 pairs no segment can pass the cut; the 16 spare entries are never used"""
    for N in (1, 100, 4096):
        assert split_entries_expected([N]) == 0 and split_cap(N) >= 16
