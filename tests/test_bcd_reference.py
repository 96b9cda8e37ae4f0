"""The numpy restatement of the reference's BCD learner (tests/bcd_ref.py) against the reference's own numbers
(tests/cpp/bcd_learner_test.cc) on tests/golden/rcv1_100.libsvm: the yardstick of learner = bcd, checked without a GPU."""
import os

import numpy as np
import pytest

import bcd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
DIAG_NEWTON = [34.877064, 33.885559, 29.572740, 27.458964, 25.317689, 23.917098, 22.855843, 22.099876, 21.552682,
               21.137216]   # bcd_learner_test.cc:19-30


@pytest.fixture(scope="module")
def data():
    return R.read_libsvm(DATA)


def test_refrand_is_glibc_rand():
    """rand() after srand(1) (the first values of glibc's default generator)"""
    s = R.RefRand()
    assert [s.next() for _ in range(3)] == [1804289383, 846930886, 1681692777]


def test_diag_newton_trajectory(data):
    m = R.BCD([data], l1=.1, lr=.05, block_ratio=.001, tail_feature_filter=0)
    assert len(m.ranges) == 1
    got = m.run(10, R.RefRand())
    for g, want in zip(got, DIAG_NEWTON):
        assert abs(g - want) / g < 1e-5, (got, DIAG_NEWTON)


@pytest.mark.parametrize("ratio,nblk", [(.4, 36), (1, 89), (10, 881)])
def test_block_counts(data, ratio, nblk):
    """ceil(entries / rows counted x block_ratio) over every 10th row; the ranges cover the key space in order"""
    st = R.fea_group_stats([(data[0], data[1])], 0)
    assert st[1] == 10 and st[2] == 100
    assert R.block_counts(st, ratio) == [(0, nblk)]
    rg = R.partition_feature(0, [(0, nblk)])
    assert len(rg) == nblk and rg[0][0] == 0 and rg[-1][1] == R.U64
    assert all(a[1] <= b[0] and b[0] - a[1] <= 1 for a, b in zip(rg, rg[1:]))


def test_partition_with_feature_groups():
    """num_feature_group_bits = 4: each group's range is ReverseBytes of its ids, the ranges are sorted and disjoint"""
    rg = R.partition_feature(4, [(1, 3), (2, 2), (7, 1)])
    assert len(rg) == 6
    assert all(a[1] <= b[0] for a, b in zip(rg, rg[1:]))
    for gid in (1, 2, 7):
        k = R.reverse_bytes((12345 << 4) | gid)
        assert sum(b <= k < e for b, e in rg) == 1


def test_convergence(data):
    """bcd_learner_test.cc:44-73: ratios .4, 1 and 10 reach the optimum 15.884923 within 1e-3 in 50 epochs, the
    shuffles drawing from one stream"""
    stream = R.RefRand()
    R.BCD([data], l1=.1, lr=.05, block_ratio=.001, tail_feature_filter=0).run(10, stream)   # DiagNewton first
    for ratio in (.4, 1, 10):
        got = R.BCD([data], l1=.1, lr=.8, block_ratio=ratio, tail_feature_filter=0).run(50, stream)
        assert abs(got[-1] - 15.884923) / got[-1] < 1e-3, (ratio, got[-1])


def test_update_weight_cases():
    """the soft threshold: inside [-l1, l1] w goes to 0, outside a clamped Newton step"""
    w = np.array([0, 0, 0, .5], np.float32)
    g = np.array([.05, 2.0, -2.0, 0], np.float32)
    h = np.array([1, 1, 1, 1], np.float32)
    nw, nd, d = R.update_weight(g, h, w, np.ones(4, np.float32), .1, 1.0)
    assert nw[0] == 0 and d[1] < 0 and d[2] > 0
    assert np.all(np.abs(d) <= 1) and np.all(nd <= 5)
