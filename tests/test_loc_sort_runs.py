"""k_loc_sort's in-wave run formation on bucket populations the C3 stream never produces.

One block sorts one bucket: every wave sorts 64 pairs of the bucket in registers (a bitonic network over the 64 lanes), then the
64-runs are merged in LDS.  The C3 stream only ever shows it buckets of 381 +- 30 pairs, so the cases here put a CHOSEN number of
pairs into ONE bucket — a lone pair, runs one short of / exactly / one over the 64 lanes, one and two full merge rounds, the LDS
capacity of 1 024 pairs — and keys that exercise each word of the 96-bit compare on its own.

How the pairs land in one bucket (dfh_localize_api.hip: localize_impl; nothing here depends on it for its RESULT, only for its coverage):
  * a first call on a batch object with N <= 192 pairs takes P = 1 bucket: the cases up to 129 pairs are one cold call;
  * the stored splitters are kept while N / P stays within [48, 700]: after a first minibatch of 100 pairs (P = 1) a minibatch of
    511 .. 513 pairs is one bucket again;
  * 1 024 pairs: a first minibatch of 300 pairs whose keys all have the top byte 0xFF leaves P = 2 and a splitter with such a
    key; a second minibatch whose keys are all smaller falls into bucket 0 as a whole (1 024 = the LDS capacity).

The one-bucket premise above is NOT asserted here (dfh_batch_get_key_view shows the bucket starts since; tests/test_key_view.py
asserts the premises of its own designs through it): it holds for LOC_MIN_AVG = 48,
LOC_MAX_AVG = 700 (dfh_localize.hip), DFH_LOC_SMALL_AVG = 192 (dfh_localize_api.hip) and splitters = the previous minibatch's quantiles; a
change to any of them turns the larger cases into ordinary multi-bucket sorts (still correct, no longer this file's subject).  A
comment next to the constants points back here.

What these cases can NOT see is the order of the tags among equal keys: U, feaids, feacnt and index are the same whichever
order equal keys end up in (all_equal gives one key and an all-zero index).  A comparator that ignored the tag would only show
here when it loses a pair.  The tie order decides the order of the key-ordered (row, value) view the update sums over: it is
pinned exactly by tests/test_key_view.py, which reads that view back, not by this file.

The expectation is numpy's stable sort of (ReverseBytes(id), position) (Localizer::Compact, localizer.cc:22-77); the CPU test
checks that expectation against the oracle's Localizer on every case, the GPU tests check the device against it.
"""
import numpy as np
import pytest

SIZES = [1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1024]
KEYS = ["random", "all_equal", "high_word_only", "low_word_only"]


def reverse_bytes(ids):
    """ReverseBytes of the reference (localizer.h): the 16 four-bit digits of the id in reverse order"""
    x = np.ascontiguousarray(ids, np.uint64).byteswap()
    lo = np.uint64(0x0F0F0F0F0F0F0F0F)
    return ((x & lo) << np.uint64(4)) | ((x >> np.uint64(4)) & lo)


def make_ids(kind, n, seed):
    """n raw ids whose keys (the digit-reversed ids) are all below 0xFF << 56"""
    rng = np.random.default_rng(seed)
    if kind == "random":   # a third of the pairs repeat a key
        ids = rng.integers(0, 2 ** 64 - 1, size=n, dtype=np.uint64)
        dup = rng.random(n) < 0.33
        ids[dup] = rng.choice(ids, size=int(dup.sum()))
    elif kind == "all_equal":   # the order is the tags' alone
        ids = np.full(n, 0x0123456789ABCD42, np.uint64)
    elif kind == "high_word_only":   # the key's high word is the id's low word, reversed; 24 distinct values: ties too
        ids = np.uint64(0x1122334400000000) | rng.integers(0, 2 ** 32, size=24, dtype=np.uint64)[rng.integers(0, 24, size=n)]
    else:   # low_word_only: the keys differ in their low word alone (the id's high word)
        ids = (rng.integers(0, 2 ** 32, size=24, dtype=np.uint64)[rng.integers(0, 24, size=n)] << np.uint64(32)) | np.uint64(0x55667742)
    ids = ids & ~np.uint64(0x8)   # lowest digit of the id = top digit of the key: at most 7
    assert int(reverse_bytes(ids).max()) < 0xFF << 56
    return ids


def make_batch(ids, seed):
    """ragged rows (some empty) over the ids"""
    rng = np.random.default_rng(seed + 1)
    n = len(ids)
    cuts = np.sort(rng.integers(0, n + 1, size=max(1, n // 3)))
    off = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
    return dict(offset=off, index=ids, value=rng.normal(size=n).astype(np.float32), label=np.ones(len(off) - 1, np.float32))


def primer(n):
    """the minibatch that leaves the splitters which put the next n pairs into one bucket (None: a cold call does)"""
    if n <= 192:
        return None
    m = 100 if n <= 700 else 300
    ids = (np.arange(m, dtype=np.uint64) << np.uint64(8)) | np.uint64(0xFF)   # keys 0xFF......: above every key of make_ids
    return make_batch(ids, 7)


def expected(b):
    keys = reverse_bytes(b["index"])
    order = np.lexsort((np.arange(len(keys)), keys))   # by key, ties by position: stable
    sk = keys[order]
    head = np.ones(len(sk), bool)
    head[1:] = sk[1:] != sk[:-1]
    rank = np.cumsum(head) - 1
    index = np.empty(len(sk), np.uint32)
    index[order] = rank
    return dict(U=int(head.sum()), feaids=sk[head], feacnt=np.bincount(rank).astype(np.float32), index=index)


def check(got, want, what):
    assert got["U"] == want["U"], what
    assert np.array_equal(got["feaids"], want["feaids"]), what
    assert np.array_equal(got["feacnt"], want["feacnt"]), what
    assert np.array_equal(got["index"], want["index"]), what


def cases():
    return [(kind, n) for kind in KEYS for n in SIZES]


@pytest.mark.parametrize("kind,n", cases())
def test_expectation_is_the_oracle_localizer(oracle, kind, n):
    """CPU: what the GPU tests assert is what the oracle's Localizer gives, primers included"""
    for b in (primer(n), make_batch(make_ids(kind, n, 100 + n), n)):
        if b is not None:
            check(oracle.localize(b["offset"], b["index"]), expected(b), (kind, n))


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


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["lds", "global"])
@pytest.mark.parametrize("kind,n", cases())
def test_one_bucket_of_n_pairs(capi, ctx, kind, n, path):
    """n pairs in one bucket, through the LDS sort (the in-wave network + merge rounds) and through the global-memory path"""
    bt = capi.Batch(ctx, 1200, 1200)
    bt.set_option("force_sort_fallback", path == "global")
    for b in (primer(n), make_batch(make_ids(kind, n, 100 + n), n)):
        if b is None:
            continue
        bt.load_host(b["offset"], b["index"], b["value"], b["label"])
        bt.localize()
        check(bt.get_localized(), expected(b), (kind, n, path, len(b["index"])))
    bt.close()


@pytest.mark.gpu
def test_same_pairs_every_order(capi, ctx):
    """the sorted order is unique: 129 pairs of 5 keys give the same dictionary and counts whatever order they arrive in"""
    rng = np.random.default_rng(3)
    base = make_ids("random", 5, 1)[rng.integers(0, 5, size=129)]
    bt = capi.Batch(ctx, 200, 200)
    for perm in (np.arange(129), np.arange(129)[::-1], rng.permutation(129), np.argsort(reverse_bytes(base), kind="stable")):
        b = make_batch(np.ascontiguousarray(base[perm]), 9)
        bt.load_host(b["offset"], b["index"], b["value"], b["label"])
        bt.localize()
        check(bt.get_localized(), expected(b), "order")
    bt.close()
