"""The kernels of learner = bcd (difacto_amd/csrc/dfh_bcd.hip) through capi.Bcd against the numpy restatement of the
reference (tests/bcd_ref.py): one block's g and h (fp64), UpdateWeight in float, the float prediction update bit for bit,
the split-key path, empty blocks, the AUC path beyond 32 768 rows and run-to-run determinism.  The step check itself
(R.check_block) and R.make_device live in tests/bcd_ref.py, shared with tests/test_bcd_shapes.py, which runs the same
check on inputs designed to sit on the kernels' share, step and chain boundaries."""
import os

import numpy as np
import pytest

import bcd_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")


@pytest.fixture(scope="module")
def capi():
    from difacto_amd import capi as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def ctx(capi):
    c = capi.Context(0)
    yield c
    c.close()


def test_block_step_matches_restatement(capi, ctx):
    d = R.read_libsvm(DATA)
    chunks = R.split_rows(*d, [30, 25, 45])
    ref = R.BCD(chunks, l1=.1, lr=.8, block_ratio=1, tail_feature_filter=0, stats=R.fea_group_stats([(d[0], d[1])], 0))
    o = R.make_device(capi, ctx, chunks, ref.ranges)
    try:
        assert o.nkeys == len(ref.keys)
        rng = np.random.default_rng(0)
        steps = 0
        for blk in list(rng.permutation(len(ref.ranges)))[:30] * 2:   # every block twice: pred and w are non-zero the 2nd time
            g = R.check_block(o, ref, int(blk))
            steps += len(g) > 0
        assert steps > 10
    finally:
        o.close()


def test_split_key_path_and_radix_auc(capi, ctx):
    """a chunk of 2^20 rows with one key in every row (its entries cross ~1000 shares) and values; AUC beyond 32 768 rows"""
    rng = np.random.default_rng(1)
    n, per = 1 << 20, 3
    ids = np.empty((n, per), np.uint64)
    ids[:, 0] = 7
    ids[:, 1:] = rng.integers(8, 3000, size=(n, per - 1))
    off = (np.arange(n + 1) * per).astype(np.uint64)
    val = rng.normal(size=n * per).astype(np.float32)
    lab = (rng.random(n) < 0.3).astype(np.float32)
    chunk = (off, ids.ravel(), val, lab)
    ranges = [(0, R.U64)]
    ref = R.BCD([chunk], l1=.1, lr=.8, block_ratio=1, tail_feature_filter=0)
    ref.ranges, ref.pos = ranges, [(0, len(ref.keys))]
    o = R.make_device(capi, ctx, [chunk], ranges)
    try:
        for _ in range(2):
            R.check_block(o, ref, 0)
        _, _, prog = o.step(0, progress=True)
        pred = o.get_pred(0)
        y = np.where(lab > 0, 1.0, -1.0)
        assert prog[0] == n
        assert abs(prog[1] - np.log1p(np.exp(-y * pred.astype(np.float64))).sum()) <= 1e-5 * prog[1]
        order = np.argsort(pred, kind="stable")
        pos = lab[order] > 0
        area = np.cumsum(pos)[~pos].sum() / (pos.sum() * (n - pos.sum()))
        assert abs(prog[2] / n - max(area, 1 - area)) < 1e-4
    finally:
        o.close()


def test_empty_blocks_and_epochs(capi, ctx):
    """block_ratio 10 on the golden data: 881 blocks for 2 775 keys, some of them empty; epochs follow the restatement"""
    d = R.read_libsvm(DATA)
    ref = R.BCD([d], l1=.1, lr=.8, block_ratio=10, tail_feature_filter=0)
    o = R.make_device(capi, ctx, [d], ref.ranges)
    try:
        info = [o.block_info(b) for b in range(len(ref.ranges))]
        empty = [b for b, i in enumerate(info) if i[2] == 0]
        assert len(empty) >= 10, len(empty)
        assert all(info[b][1] - info[b][0] == 0 for b in empty)
        w0 = o.get_model()["w"].copy()
        p0 = o.get_pred(0).copy()
        o.step(empty[0])
        assert np.array_equal(o.get_model()["w"], w0) and np.array_equal(o.get_pred(0), p0)
        stream = R.RefRand()
        order = list(range(len(ref.ranges)))
        got = []
        for ep in range(3):
            stream.shuffle(order)   # the order persists from epoch to epoch and is shuffled again
            prog = o.epoch(order)
            assert prog[0] == 100
            got.append(prog[1])
        want = ref.run(3, R.RefRand())
        assert np.allclose(got, want, rtol=1e-5, atol=0), (got, want)
    finally:
        o.close()


def test_epochs_are_deterministic(capi, ctx):
    d = R.read_libsvm(DATA)
    chunks = R.split_rows(*d, [50, 50])
    ranges = R.partition_feature(0, [(0, 7)])
    out = []
    for _ in range(2):
        o = R.make_device(capi, ctx, chunks, ranges, val=[chunks[0]])
        try:
            progs = [o.epoch([3, 1, 6, 0, 2, 5, 4]) for _ in range(3)]
            out.append((np.array(progs), o.get_model()["w"], o.get_pred(0), o.get_pred(0, is_val=True)))
        finally:
            o.close()
    for a, b in zip(*out):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
