"""k_loc_scatter derives the bucket, the slot and the row of every pair itself: the Localizer's full outputs, exactly.

The count pass hands the scatter pass one array, the offsets of the (tile, bucket) runs.  The scatter pass repeats count's
splitter search for the bucket, deals out the slots of a run with an LDS cursor, and finds the row of a position in the CSR
offsets: the tile's first row by one search per tile, the offsets of up to LOC_SCATTER_ROWS = 1 024 rows from there staged in
LDS and searched per pair, a search of `offset` in global memory for a tile that spans more rows.  The cases below are the
smallest minibatches that reach every branch of that: empty rows at the start, inside and at the end; rows across and on the
borders of the 2 048-pair tiles; tiles of more than 1 024 rows; one row over several tiles; the second call on a batch
object, whose splitters are pairs of this very minibatch; one key in every bucket; one pair; the large size class; the count
pass that gathers a described minibatch.

Every case is localized twice on one batch object (bootstrapped splitters, then the exact quantiles the first call left) and
compared each time with the oracle Localizer (feaids, feacnt, index) and with tests/keyview_ref.py (col_ptr, s_row, s_val,
the segment lists); the bucket starts of the second call are the ones the exact quantiles give, which checks the splitters
the first call wrote.  Every comparison is exact.
"""
import numpy as np
import pytest

import keyview_ref as K

gpu = pytest.mark.gpu
TILE = 2048           # dfh_feed_layout.h: LOC_TILE
STAGED_ROWS = 1024    # dfh_localize.hip: LOC_SCATTER_ROWS
SMALL_CLASS_PAIRS = 701 * 1024   # localize_impl: N / 1024 <= 700 keeps the small size class
KW = dict(l1=0.01, l2=0.0, lr=0.1, seed=3)


# ------------------------------------------------------------------------------------------------ the minibatches
def from_row_lens(row_lens, seed, key_space, binary=False):
    rng = np.random.default_rng(seed)
    row_lens = np.asarray(row_lens, np.int64)
    off = np.concatenate([[0], np.cumsum(row_lens)]).astype(np.uint64)
    N = int(off[-1])
    ranks = rng.integers(0, key_space, size=N).astype(np.uint64)
    ids = K.reverse_bytes((ranks + np.uint64(1)) << np.uint64(K.SHIFT))
    val = None if binary else rng.normal(size=N).astype(np.float32)
    lab = np.where(rng.random(len(row_lens)) < 0.4, 1.0, 0.0).astype(np.float32)
    return dict(offset=off, index=ids, value=val, label=lab)


def empty_rows_lens():
    """rows of 0 .. 8 pairs, about 3 000 pairs (two tiles): empty rows first, last, and in runs; the row that holds position
    2 048 stands between two runs of empty rows"""
    rng = np.random.default_rng(11)
    head = rng.integers(0, 9, size=2000)
    head[:5] = 0
    for at in (100, 300, 301):
        head[at:at + 6] = 0
    k = int(np.searchsorted(np.cumsum(head), TILE - 10))     # the head ends at 2 038 .. 2 046 pairs
    tail = rng.integers(0, 9, size=250)
    tail[120:126] = 0
    tail[-7:] = 0
    return np.concatenate([head[:k + 1], [0, 0, 0, 20, 0, 0, 0, 0], tail])


def long_row_lens(n_tiles):
    """N just over n_tiles * 2 048 with one long row across the last border, rows of 1 .. 5 before it and a few after it"""
    rng = np.random.default_rng(12 + n_tiles)
    before = []
    while sum(before) < n_tiles * TILE - 40:
        before.append(int(rng.integers(1, 6)))
    before[-1] -= sum(before) - (n_tiles * TILE - 40)
    return np.array(before + [0, 70, 0, 3, 4])               # the long row covers [border - 40, border + 30)


def border_on_row_start_lens():
    """a row starts exactly at position 2 048 — behind two empty rows that share its offset — and another at 4 096"""
    rng = np.random.default_rng(14)
    out, at = [], 0
    for border in (TILE, 2 * TILE):
        while at < border - 9:
            n = int(rng.integers(1, 9))
            out.append(n)
            at += n
        out.append(border - at)
        at = border
        out += [0, 0] if border == TILE else []
    return np.array(out + [5, 0, 2])


CASES = {
    "empty_rows": lambda: from_row_lens(empty_rows_lens(), 1, 700),
    "long_row_over_2048": lambda: from_row_lens(long_row_lens(1), 2, 500, binary=True),
    "long_row_over_4096": lambda: from_row_lens(long_row_lens(2), 3, 900),
    "border_on_row_start": lambda: from_row_lens(border_on_row_start_lens(), 4, 900),
    # 3 000 one-pair rows (tiles of 2 048 rows: the search in global memory), then rows of 60 (staged again), empty last rows
    "wide_tiles": lambda: from_row_lens([0] * 3 + [1] * 3000 + [60] * 40 + [0] * 4, 5, 1200),
    # a tile of exactly as many rows as are staged, and of one more
    "staged_rows_edge": lambda: from_row_lens([1] * (STAGED_ROWS - 1) + [TILE - (STAGED_ROWS - 1)] + [1] * STAGED_ROWS
                                              + [TILE - STAGED_ROWS] + [2, 2], 6, 800, binary=True),
    "one_row_three_tiles": lambda: from_row_lens([5000], 7, 1500),
    "all_ids_equal": lambda: from_row_lens(np.random.default_rng(8).integers(0, 7, size=1700), 8, 1),
    "one_pair": lambda: from_row_lens([0, 0, 1, 0], 9, 1),
    "below_one_bucket": lambda: from_row_lens([0, 30, 0, 0, 41, 29], 10, 40),
    # the large size class: just above the pairs the small one takes, rows of 0 .. 20
    "large_class": lambda: from_row_lens(large_class_lens(), 13, 300000),
}


def large_class_lens():
    rng = np.random.default_rng(15)
    lens = rng.integers(0, 21, size=73000)
    n = np.cumsum(lens)
    rows = int(np.searchsorted(n, SMALL_CLASS_PAIRS + 700)) + 1
    return lens[:rows]


_MB = {}


def case(name, oracle, bounds):
    """(minibatch, oracle Localizer output, reference key view): computed once"""
    if name not in _MB:
        mb = CASES[name]()
        loc = oracle.localize(mb["offset"], mb["index"])
        _MB[name] = (mb, loc, K.reference(mb["offset"], loc["index"], mb["value"], bounds))
    return _MB[name]


# ------------------------------------------------------------------------------------------------ CPU: the designs hold
def test_designs_reach_the_edges():
    lens = empty_rows_lens()
    off = np.concatenate([[0], np.cumsum(lens)])
    assert TILE < off[-1] < 2 * TILE and lens[0] == 0 and lens[-1] == 0
    r = int(np.searchsorted(off, TILE, side="right")) - 1   # last row that starts at or before 2 048
    assert lens[r] > 0 and lens[r - 1] == 0 and lens[r + 1] == 0
    for t in (1, 2):
        lens = long_row_lens(t)
        off = np.concatenate([[0], np.cumsum(lens)])
        assert t * TILE < off[-1] < t * TILE + 64 and np.any((off[:-1] < t * TILE) & (off[1:] > t * TILE) & (lens == 70))
    off = np.concatenate([[0], np.cumsum(border_on_row_start_lens())])
    assert (off == TILE).sum() == 3 and (off == 2 * TILE).sum() == 1 and off[-1] > 2 * TILE
    mb = CASES["wide_tiles"]()
    rows_in_tile0 = int(np.searchsorted(mb["offset"], TILE, side="right"))
    assert rows_in_tile0 > STAGED_ROWS and int(mb["offset"][-1]) > 2 * TILE
    off = CASES["staged_rows_edge"]()["offset"].astype(np.int64)
    per_tile = [int(np.searchsorted(off, (t + 1) * TILE - 1, side="right") - (np.searchsorted(off, t * TILE, side="right") - 1))
                for t in range(2)]
    assert per_tile == [STAGED_ROWS, STAGED_ROWS + 1]
    assert len(np.unique(CASES["all_ids_equal"]()["index"])) == 1 and int(CASES["all_ids_equal"]()["offset"][-1]) > 20 * K.SMALL_AVG
    assert int(CASES["one_pair"]()["offset"][-1]) == 1 and int(CASES["below_one_bucket"]()["offset"][-1]) < K.SMALL_AVG
    n = int(np.sum(large_class_lens()))
    assert SMALL_CLASS_PAIRS < n < SMALL_CLASS_PAIRS + 1000


# ------------------------------------------------------------------------------------------------ GPU
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


@pytest.fixture(scope="module")
def bounds(capi, ctx):
    bt = capi.Batch(ctx, 2, 4)
    bt.load_host(np.array([0, 2, 3], np.uint64), np.array([5, 5, 9], np.uint64), None, np.ones(2, np.float32))
    bt.localize()
    v = bt.get_key_view()
    bt.close()
    return {k: v[k] for k in ("BWD_SMALL", "BWD_MID", "HOT_SPLIT", "HOT_SPLIT_MIN")}


def outputs(bt):
    return bt.get_localized(), bt.get_key_view()


def check(out, loc, ref, stored):
    """the Localizer's outputs against the oracle's and the reference view; stored: the bucket starts are the ones the
    exact quantiles of this minibatch give"""
    got, view = out
    assert got["U"] == loc["U"]
    assert np.array_equal(got["feaids"], loc["feaids"]), "feaids"
    assert np.array_equal(got["feacnt"].view(np.uint32), np.asarray(loc["feacnt"], np.float32).view(np.uint32)), "feacnt"
    assert np.array_equal(got["index"], loc["index"]), "index"
    assert view["P"] > 0, "not the sample sort"
    K.check_key_view(view, ref, split="skip")
    if stored:
        assert np.array_equal(view["bstart"], K.stored_bstart(ref["s_row"], ref["nnz"], view["P"])), "bucket starts of the second call"


def localize_twice(capi, ctx, mb, loc, ref):
    bt = capi.Batch(ctx, len(mb["label"]), int(mb["offset"][-1]))
    try:
        outs = []
        for rnd in range(2):
            bt.load_host(mb["offset"], mb["index"], mb["value"], mb["label"])
            bt.localize()
            outs.append(outputs(bt))
            check(outs[-1], loc, ref, stored=(rnd == 1))
        assert outs[0][1]["P"] == outs[1][1]["P"]
        return outs
    finally:
        bt.close()


@gpu
@pytest.mark.parametrize("name", [n for n in CASES if n != "large_class"])
def test_small_class(capi, ctx, oracle, bounds, name):
    """bootstrapped splitters, then the minibatch's own exact quantiles: a splitter pair sits in a row that is no multiple
    of 2^tb wherever row 0 is empty, and in row 0 — a multiple — in the one-row minibatch"""
    mb, loc, ref = case(name, oracle, bounds)
    first, _ = localize_twice(capi, ctx, mb, loc, ref)
    N = int(mb["offset"][-1])
    assert first[1]["P"] == K.cold_buckets(N)
    if name == "all_ids_equal":
        assert loc["U"] == 1 and first[1]["P"] > 20


def same_bytes(a, b):
    for k in ("feaids", "feacnt", "index"):
        assert a[0][k].tobytes() == b[0][k].tobytes(), k
    for k in ("col_ptr", "s_row", "s_val", "bstart"):
        assert a[1][k].tobytes() == b[1][k].tobytes(), k
    for k in ("few", "mid", "hot"):      # a bucket's entries are listed in the order its threads arrive: compared as sets
        assert np.array_equal(a[1][k]["desc"], b[1][k]["desc"]), k
        for x, y in zip(a[1][k]["buckets"], b[1][k]["buckets"]):
            assert np.array_equal(K._rows_sorted(x), K._rows_sorted(y)), k


@gpu
def test_large_class_and_determinism(capi, ctx, oracle, bounds):
    """the 4 096-bucket tables (12 row bits in the tag: rows 4 096, 8 192, ... have low bits 0), and two runs of the same
    minibatch on two batch objects give identical bytes"""
    mb, loc, ref = case("large_class", oracle, bounds)
    a = localize_twice(capi, ctx, mb, loc, ref)
    assert a[1][1]["P"] > 1024
    b = localize_twice(capi, ctx, mb, loc, ref)
    same_bytes(a[1], b[1])        # the second calls: both on the exact quantiles


@gpu
def test_device_feed(capi, ctx, oracle, bounds):
    """a described minibatch (dfh_batch_prepare_rows): the second call's count pass gathers the rows out of the row buffer
    itself; rows taken in another order than the buffer's, empty rows among them"""
    src = CASES["empty_rows"]()
    nrows_src = len(src["label"])
    rng = np.random.default_rng(21)
    rows = rng.permutation(nrows_src)[:700].astype(np.uint32)
    so = src["offset"].astype(np.int64)
    lens = (so[1:] - so[:-1])[rows]
    assert lens[:60].min() == 0 and lens.sum() > TILE
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    take = np.concatenate([np.arange(so[r], so[r + 1]) for r in rows]).astype(np.int64)
    mb = dict(offset=off, index=src["index"][take], value=src["value"][take], label=src["label"][rows])
    loc = oracle.localize(mb["offset"], mb["index"])
    ref = K.reference(mb["offset"], loc["index"], mb["value"], bounds)
    N = int(off[-1])
    rb = capi.RowBuf(ctx, nrows_src, int(so[-1]))
    bt = capi.Batch(ctx, len(rows), N)
    tb = capi.Table(ctx, 1 << 15, V_dim=0, **KW)
    try:
        rb.load_host(src["offset"], src["index"], src["value"])
        for rnd in range(2):
            bt.prepare_rows(tb, mb["offset"], mb["label"], [(rb, rows)])
            bt.sgd_step(tb, is_train=True, push_cnt=(rnd == 0))
            check(outputs(bt), loc, ref, stored=(rnd == 1))
            o, lab = bt.get_rows()
            assert np.array_equal(o, mb["offset"].astype(np.uint32)) and np.array_equal(lab, mb["label"])
        tb.check()
    finally:
        for o in (bt, rb, tb):
            o.close()
