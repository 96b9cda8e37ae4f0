"""The resident chunk set behind learner = lbfgs and learner = bcd (difacto_amd/csrc/dfh_chunks.hip): both objects make a
reader block resident, merge the chunks' feature counts and map every chunk's keys onto the model through the same code.

The designed data (12 training rows, 1 validation row, 8 ids; tail_feature_filter = 3), counts per chunk:

  id   T0 (values)   T1 (binary)   merged
  A    2             1             3 = the filter exactly: dropped
  B    2             2             4 = the filter + 1: kept
  C    -             5             5   only in the second chunk
  D    6             -             6
  E    1             1             2   dropped
  F    4             -             4
  H    3             3             6
  G    only in the validation chunk (one row: B, G, D): never a key of the model

T0 has a row without entries, T1 has no values, the validation chunk is a single row.  Values and weights are small
integers and powers of two, so every prediction is exact in float whatever the order of the adds.

The cut of a reader block at the entry bound (ForEachChunk, difacto_amd/host/resident_data.h) is checked without a GPU
by the host-only cases of build/difacto_host_tests."""
import os
import subprocess

import numpy as np
import pytest

import bcd_ref as R

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
ERR_ARG = 1   # DFH_ERR_ARG, include/difacto_hip.h

A, B, C, D, E, F, G, H = 1, 2, 3, 4, 5, 6, 7, 8
FILTER = 3
ALL_KEYS = [(0, (1 << 64) - 1)]   # one block over every key


def _chunk(rows, binary, seed):
    """rows: the ids of every row -> (offset, index, value or None, label); values in {1, 2, 3}"""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    idx = np.array([i for r in rows for i in r], np.uint64)
    val = None if binary else rng.integers(1, 4, size=len(idx)).astype(np.float32)
    lab = np.where(np.arange(len(rows)) % 2 == 0, 1.0, -1.0).astype(np.float32)
    return off, idx, val, lab


T0 = _chunk([[A, B, D, F, H], [A, B, D, F, H], [D, E, F, H], [], [D, F], [D], [D]], False, 1)
T1 = _chunk([[A, B, C, H], [B, C, E, H], [C, H], [C], [C]], True, 2)
V0 = _chunk([[B, G, D]], False, 3)


def merged_counts(train):
    """KVUnion of the chunks' (key, count) pairs: float32 counts added in chunk order; keys ascending"""
    tot = {}
    for off, idx, _, _ in train:
        keys, cnt = np.unique(R.reverse_bytes_np(idx), return_counts=True)
        for k, c in zip(keys, cnt.astype(np.float32)):
            tot[int(k)] = np.float32(tot.get(int(k), np.float32(0)) + c)
    keys = np.array(sorted(tot), np.uint64)
    return keys, np.array([tot[int(k)] for k in keys], np.float32)


def model_of(train, tail):
    keys, cnt = merged_counts(train)
    keep = cnt > np.float32(tail)
    return keys[keep], cnt[keep]


def preds(chunk, keys, w):
    """pred of every row from w, keys outside the model skipped; exact for this file's values and weights"""
    off, idx, val, _ = chunk
    rk = R.reverse_bytes_np(idx)
    pos = np.searchsorted(keys, rk)
    hit = (pos < len(keys)) & (keys[np.minimum(pos, len(keys) - 1)] == rk)
    term = np.where(hit, w[np.minimum(pos, len(keys) - 1)], 0).astype(np.float64) * (1.0 if val is None else val)
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
    return np.bincount(rows, weights=term, minlength=len(off) - 1).astype(np.float32)


def identical(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_design_holds():
    keys, cnt = merged_counts([T0, T1])
    by_id = {i: float(cnt[list(keys).index(R.reverse_bytes(i))]) for i in (A, B, C, D, E, F, H)}
    assert by_id[A] == FILTER and by_id[B] == FILTER + 1
    assert C not in T0[1] and C in T1[1]
    assert R.reverse_bytes(G) not in keys and G in V0[1]
    assert 0 in np.diff(T0[0].astype(np.int64)) and T1[2] is None and len(V0[3]) == 1
    mk, mc = model_of([T0, T1], FILTER)
    assert sorted(mk) == sorted(R.reverse_bytes(i) for i in (B, C, D, F, H)) and len(mk) < len(keys)


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


def _logit_objv(chunks, keys, w):
    return sum(float(np.logaddexp(0, -np.where(c[3] > 0, 1.0, -1.0) * preds(c, keys, w).astype(np.float64)).sum()) for c in chunks)


@gpu
def test_lbfgs_and_bcd_merge_the_same_chunks_alike(capi, ctx):
    lb, bc = capi.Lbfgs(ctx, 0, 3), capi.Bcd(ctx)
    try:
        for o in (lb, bc):
            o.add_chunk(*T0)
            o.add_chunk(*T1)
            o.add_chunk(*V0, is_val=True)
        nkeys, n = lb.init_model(tail_feature_filter=FILTER)
        assert bc.build(ALL_KEYS, tail_feature_filter=FILTER) == nkeys == n
        ml, mb = lb.get_model(), bc.get_model()
        want_keys, want_cnt = model_of([T0, T1], FILTER)
        assert np.array_equal(ml["keys"], mb["keys"]) and R.same_bits(ml["cnt"], mb["cnt"])
        assert np.array_equal(ml["keys"], want_keys) and R.same_bits(ml["cnt"], want_cnt)
        assert bc.block_info(0)[:2] == (0, nkeys)
        # every chunk's keys land on their model positions (filtered and unknown keys on none): predictions from a w
        # of distinct powers of two, exact in float
        w = (2.0 ** np.arange(-2, len(want_keys) - 2)).astype(np.float32)
        assert bc.set_model(want_keys, w) == nkeys
        for i, c in enumerate((T0, T1)):
            assert R.same_bits(bc.get_pred(i), preds(c, want_keys, w))
        assert R.same_bits(bc.get_pred(0, is_val=True), preds(V0, want_keys, w))
        # the same through L-BFGS's gather: the objective of the training chunks at w.  The predictions are exact; the
        # float loss of a row is a few ulp (6e-8) off, summed over 12 rows in fp64: the 1e-5 of test_lbfgs_state
        lb.set_weights(w)
        loss, _ = lb.calc_grad()
        want = _logit_objv([T0, T1], want_keys, w)
        print("lbfgs objective %.9g, numpy %.9g" % (loss, want))
        assert abs(loss - want) <= 1e-5 * abs(want)
    finally:
        lb.close()
        bc.close()


@gpu
def test_add_chunk_is_refused_once_the_model_stands(capi, ctx):
    lb, bc = capi.Lbfgs(ctx, 0, 3), capi.Bcd(ctx)
    try:
        lb.add_chunk(*T0)
        bc.add_chunk(*T0)
        lb.init_model(tail_feature_filter=FILTER)
        bc.build(ALL_KEYS, tail_feature_filter=FILTER)
        with pytest.raises(capi.DfhError) as e:
            lb.add_chunk(*T1)
        assert e.value.code == ERR_ARG and "dfh_lbfgs_add_chunk: the model is already initialised" in str(e.value)
        with pytest.raises(capi.DfhError) as e:
            bc.add_chunk(*T1)
        assert e.value.code == ERR_ARG and "dfh_bcd_add_chunk: the layouts are already built" in str(e.value)
    finally:
        lb.close()
        bc.close()


@gpu
def test_a_refused_chunk_leaves_the_object_usable(capi, ctx):
    """a chunk without rows fails the argument check; the object then takes a good chunk and gives what the good chunk
    alone gives"""
    no_rows = (np.zeros(1, np.uint64), np.zeros(0, np.uint64), None, np.zeros(0, np.float32))
    got = {}
    for first_bad in (True, False):
        lb, bc = capi.Lbfgs(ctx, 0, 3), capi.Bcd(ctx)
        try:
            for o, name in ((lb, "dfh_lbfgs_add_chunk"), (bc, "dfh_bcd_add_chunk")):
                if first_bad:
                    with pytest.raises(capi.DfhError) as e:
                        o.add_chunk(*no_rows)
                    assert e.value.code == ERR_ARG and name + ": bad argument" in str(e.value)
                o.add_chunk(*T0)
            lb.init_model(tail_feature_filter=1)
            bc.build(ALL_KEYS, tail_feature_filter=1, l1=.01)
            ml, mb = lb.get_model(), bc.get_model()
            g, h, prog = bc.step(0, grad=True, progress=True)
            got[first_bad] = dict(lk=ml["keys"], lc=ml["cnt"], loss=np.float32(lb.calc_grad()[0]), bk=mb["keys"], bc=mb["cnt"], g=g, h=h,
                                  prog=prog, w=bc.get_model()["w"], pred=bc.get_pred(0))
        finally:
            lb.close()
            bc.close()
    want_keys, want_cnt = model_of([T0], 1)
    assert np.array_equal(got[False]["lk"], want_keys) and R.same_bits(got[False]["lc"], want_cnt)
    assert np.any(got[False]["w"] != 0)
    for name in got[False]:
        assert identical(got[True][name], got[False][name]), name


def test_reader_block_is_cut_at_the_entry_bound():
    """ForEachChunk with a bound of 10 entries on hand-made blocks, in the host-only cases of the host test binary"""
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    r = subprocess.run([os.path.join(ROOT, "build", "difacto_host_tests"), DATA, "reader"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "[  OK  ] ForEachChunk cuts a block at the entry bound" in r.stdout
