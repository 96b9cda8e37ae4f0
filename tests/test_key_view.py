"""The Localizer's second product — the key-ordered view and the segment lists — compared exactly with tests/keyview_ref.py.

What the backward and the update pass walk (col_ptr, s_row, s_val; the few / mid / hot lists; the split list a training step
adds) is read back with Batch.get_key_view() and compared bit for bit with a numpy restatement, on minibatches DESIGNED in
key order so that segments of every class meet the bucket cuts, the chunk boundaries of emit and the end of the minibatch in
every way, through every path that builds the view: the sample sort with bootstrapped (cold), exact (stored) and foreign
(stale) splitters, its global-memory sort (fallback), the library sort (radix), the host-built view (host), emit with the
key-index probe folded in (probe), the gathering count pass (prepare_cached) and the single-queue step.

The CPU tests check the restatement against plain loops and every design against the properties it claims.  Every
comparison is exact; there is no tolerance in this file.
"""
import numpy as np
import pytest

import keyview_ref as K

gpu = pytest.mark.gpu
NOMINAL = dict(BWD_SMALL=8, BWD_MID=64, HOT_SPLIT=1024, HOT_SPLIT_MIN=4096)   # CPU design checks only: the GPU tests ask the library
OTHER = dict(BWD_SMALL=4, BWD_MID=48, HOT_SPLIT=512, HOT_SPLIT_MIN=1024)
PATHS = ["cold", "stored", "stale", "fallback", "radix", "host", "probe"]
ONE_KEY_N = lambda b: [1, 2, b["BWD_SMALL"], b["BWD_SMALL"] + 1, b["BWD_MID"], b["BWD_MID"] + 1, 300, 1025, b["HOT_SPLIT_MIN"],
                       b["HOT_SPLIT_MIN"] + 1, 5 * b["HOT_SPLIT"], 5 * b["HOT_SPLIT"] + 1]
MIXED = lambda b: [2 * b["HOT_SPLIT_MIN"], b["BWD_SMALL"] + 1, 1, 1, b["HOT_SPLIT_MIN"], b["HOT_SPLIT_MIN"] + 1]


# ------------------------------------------------------------------------------------------------ the designs
def worst_lens(bounds, which):
    """every key exactly L times, about 6 000 pairs, not a multiple of 192"""
    L = [2, bounds["BWD_SMALL"] + 1, bounds["BWD_MID"] + 1][which]
    n = 6000 // L + 1
    if (n * L) % K.SMALL_AVG == 0:
        n += 1
    return [L] * n


def ragged_rows_batch(seed=23):
    """40 000 rows of 0 .. 4 pairs with empty first rows, empty last rows and runs of empty rows; 65 536 < N <= 131 072, so
    the sort's tags keep 15 row bits and the rows beyond 32 768 have two candidates"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 5, size=40000)
    lens[:7] = 0
    lens[-9:] = 0
    for at in (100, 20000, 32760, 39000):
        lens[at:at + 40] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    N = int(off[-1])
    ranks = rng.integers(0, 20000, size=N).astype(np.uint64)
    ranks[rng.random(N) < 0.02] = 77                     # one hot key beside the short ones
    return dict(offset=off, index=K.reverse_bytes((ranks + np.uint64(1)) << np.uint64(K.SHIFT)), value=rng.normal(size=N).astype(np.float32),
                label=np.where(rng.random(40000) < 0.5, 1.0, -1.0).astype(np.float32))


def hashed_batch(seed=31, N=3000):
    """distinct raw ids: under max_index the runs are made by collisions, a key's occurrences come from different raw ids"""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(1 << 20)[:N].astype(np.uint64) * np.uint64(2654435761) + np.uint64(12345)
    assert len(np.unique(ids)) == N
    off = np.concatenate([[0], np.sort(rng.integers(0, N + 1, size=499)), [N]]).astype(np.uint64)
    return dict(offset=off, index=ids, value=rng.normal(size=N).astype(np.float32), label=np.ones(500, np.float32))


def numpy_localize(mb, max_index=2 ** 64 - 1):
    """Localizer::Compact's index by numpy: rank of ReverseBytes(id % max_index) among the minibatch's keys"""
    ids = mb["index"] if max_index == 2 ** 64 - 1 else mb["index"] % np.uint64(max_index)
    return np.unique(K.reverse_bytes(ids), return_inverse=True)[1].astype(np.uint32)


def seg_set(ref):
    return {(int(b), int(e)) for b, e in zip(ref["col_ptr"][:-1], ref["col_ptr"][1:])}


# ------------------------------------------------------------------------------------------------ CPU: the reference, the designs
@pytest.mark.parametrize("bounds", [dict(BWD_SMALL=2, BWD_MID=4, HOT_SPLIT=3, HOT_SPLIT_MIN=7), NOMINAL])
def test_reference_against_plain_loops(bounds):
    rng = np.random.default_rng(1)
    for trial in range(60):
        nrows = int(rng.integers(1, 12))
        lens = rng.integers(0, 9, size=nrows)
        off = np.concatenate([[0], np.cumsum(lens)])
        N = int(off[-1])
        U = int(rng.integers(1, 6))
        cidx = np.unique(rng.integers(0, U, size=N), return_inverse=True)[1] if N else np.zeros(0, np.int64)
        if N and trial % 3 == 0:
            cidx[:] = 0 if trial % 2 else cidx           # one key holding everything: passes HOT_SPLIT_MIN of the tiny bounds
        val = None if trial % 4 == 0 else rng.normal(size=N).astype(np.float32)
        K.same_reference(K.reference(off, cidx, val, bounds), K.brute_force(off, cidx, val, bounds))
    one = K.batch_from_lens([5 * bounds["HOT_SPLIT"] + 1, 3, 1], 2)
    if int(one["offset"][-1]) < 20000:
        K.same_reference(K.reference(one["offset"], one["cidx"], one["value"], bounds),
                         K.brute_force(one["offset"], one["cidx"], one["value"], bounds))


def test_reference_split_parts():
    b = NOMINAL
    want = [0] * 8 + [0, 5, 5, 6]
    for n, w in zip(ONE_KEY_N(b), want):
        mb = K.batch_from_lens([n], n)
        ref = K.reference(mb["offset"], mb["cidx"], mb["value"], b)
        assert len(ref["split"]) == w
        if w:
            s = ref["split"].astype(np.int64)
            assert s[0, 1] == 0 and s[-1, 2] == n and np.all(s[1:, 1] == s[:-1, 2]) and np.all(s[:, 2] - s[:, 1] <= b["HOT_SPLIT"])
            assert np.array_equal(s[:, 3], np.arange(w) << 16 | w)
    mb = K.batch_from_lens(MIXED(b), 4)
    assert len(K.reference(mb["offset"], mb["cidx"], mb["value"], b)["split"]) == 8 + 5


@pytest.mark.parametrize("bounds", [NOMINAL, OTHER])
def test_designs_hold(bounds):
    S, M = bounds["BWD_SMALL"], bounds["BWD_MID"]
    six = [1, 2, S, S + 1, M, M + 1]
    cls = lambda n: "none" if n == 1 else "few" if n <= S else "mid" if n <= M else "hot"
    # class edges: every one of the six lengths is the first key and the last key in some case, and sits inside in all
    for first in range(6):
        for last in range(6):
            lens = K.class_edge_lens(bounds, first, last)
            assert lens[0] == six[first] and lens[-1] == six[last] and set(six) <= set(lens[1:-1])
            assert K.cold_buckets(sum(lens)) >= 2                          # more than one bucket
    assert {cls(n) for n in six} == {"none", "few", "mid", "hot"}       # "a segment of every class ends the minibatch"
    tail = K.class_edge_lens(bounds, 0, 0, lone_tail=True)
    assert tail[-1] == 1 and tail[-2] == M + 1
    # bucket stitching
    B = K.SMALL_AVG
    for ending in ("inside_run", "single"):
        L = K.stitch_layout(bounds, ending)
        m, cut = L.marks, L.cuts
        assert sum(L.lens) == 16 * B and K.cold_buckets(16 * B) == 16
        mb = K.batch_from_lens(L.lens, 5)
        ref = K.reference(mb["offset"], mb["cidx"], mb["value"], bounds)
        assert mb["offset"][1] == 0 and np.array_equal(K.stored_bstart(ref["s_row"], 16 * B, 16), cut)   # row 0 is empty
        segs = seg_set(ref)
        assert all(v in segs for v in m.values())
        assert m["ends_on_cut"][1] == cut[1] and m["begins_on_cut"][0] == cut[1]
        assert m["pair_1_1"] == (cut[2] - 1, cut[2] + 1)
        assert m["mid_S_1"] == (cut[3] - S, cut[3] + 1) and m["mid_1_S"] == (cut[4] - 1, cut[4] + S)
        assert m["hot_straddles"][0] < cut[5] < m["hot_straddles"][1] and m["hot_straddles"][1] - m["hot_straddles"][0] == M + 1
        a, e = m["three_whole_buckets"]
        assert cut[6] < a < cut[7] and cut[10] < e < cut[11]                    # buckets 7, 8, 9 hold no head
        assert m["two_whole_buckets"] == (cut[11], cut[13])
        if ending == "inside_run":
            a, e = m["open_at_the_end"]
            assert e == 16 * B and cut[13] < a < cut[14]                       # began two buckets before the last one
        else:
            assert m["last_single"] == (16 * B - 1, 16 * B) and m["before_the_single"][1] - m["before_the_single"][0] > M
    # worst legal list shape
    for which in range(3):
        lens = worst_lens(bounds, which)
        assert len(set(lens)) == 1 and sum(lens) % B and 5800 < sum(lens) < 6300
        assert cls(lens[0]) == ["few", "mid", "hot"][which]
    # chunk carry: runs across the chunk boundaries of emit, inside the buckets the stale primer cuts
    L, sizes = K.chunk_carry_layout()
    starts = np.concatenate([[0], np.cumsum(sizes)])
    assert any(600 <= n <= 900 for n in sizes) and max(sizes) > K.LDS_CAP and sizes.count(0) >= 3
    crossing = {"pair_255_1": (2, 256), "nine_over_512": (2, 512), "twelve_over_768": (2, 768), "run_300_over_two_chunks": (4, 256),
                "pair_767_1": (4, 768), "nine_over_1024": (4, 1024)}
    for name, (q, chunk) in crossing.items():
        a, e = L.marks[name]
        assert starts[q] <= a and e <= starts[q + 1] and a - starts[q] < chunk < e - starts[q], name
    a, e = L.marks["run_300_over_two_chunks"]
    assert e - a == 300 and a - starts[4] < 256 and e - starts[4] > 512
    assert L.marks["pair_255_1"] == (255, 257) and L.marks["pair_767_1"][0] - starts[4] == 767


@pytest.mark.parametrize("bounds", [NOMINAL, OTHER])
def test_stale_primers_cut_where_designed(bounds):
    """the exact quantiles of a primer, applied the way the count pass does, give the designed bucket starts"""
    L, sizes = K.chunk_carry_layout()
    designs = [(L.lens, sizes)]
    for lens in (K.class_edge_lens(bounds, 5, 2), K.class_edge_lens(bounds, 0, 0, lone_tail=True), worst_lens(bounds, 0),
                 worst_lens(bounds, 1), worst_lens(bounds, 2), K.stitch_layout(bounds, "single").lens):
        designs.append((lens, K.generic_stale_sizes(lens)))
    for lens, sizes in designs:
        N, P = int(np.sum(lens)), len(sizes)
        assert P == K.cold_buckets(N) and sum(sizes) == N
        if P >= 4:
            assert sizes.count(0) >= 2
        if N >= 2400:
            assert max(sizes) > K.LDS_CAP
        pr = K.stale_primer(lens, sizes, 3)
        assert int(pr["offset"][-1]) == N
        mine = np.sort(K.reverse_bytes(K.batch_from_lens(lens, 1)["index"]))
        theirs = np.sort(K.reverse_bytes(pr["index"]))
        assert not set(mine.tolist()) & set(theirs.tolist())
        assert np.array_equal(K.buckets_of(mine, theirs, P), np.concatenate([[0], np.cumsum(sizes)]))


def test_designed_index_is_the_oracles(oracle):
    """the compact index every design claims (rank in designed order) is what Localizer::Compact gives, and numpy_localize
    restates the hashed case"""
    L, _ = K.chunk_carry_layout()
    for lens in (K.class_edge_lens(NOMINAL, 3, 4), K.stitch_layout(NOMINAL, "inside_run").lens, L.lens, [300], MIXED(NOMINAL)):
        mb = K.batch_from_lens(lens, 9, special_values=True)
        loc = oracle.localize(mb["offset"], mb["index"])
        assert loc["U"] == len(lens) and np.array_equal(loc["index"], mb["cidx"])
        assert np.array_equal(loc["feacnt"], np.asarray(lens, np.float32))
    for mx in (7, 1000):
        mb = hashed_batch()
        loc = oracle.localize(mb["offset"], mb["index"], mx)
        assert np.array_equal(loc["index"], numpy_localize(mb, mx))
        assert loc["U"] == (7 if mx == 7 else loc["U"]) and loc["U"] <= mx and loc["feacnt"].max() > 1
    mb = ragged_rows_batch()
    N = int(mb["offset"][-1])
    assert 65536 < N <= 131072 and mb["offset"][7] == 0 and mb["offset"][-10] == N
    assert np.array_equal(oracle.localize(mb["offset"], mb["index"])["index"], numpy_localize(mb))


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
    """the class bounds the library was built with, as the accessor reports them"""
    bt = capi.Batch(ctx, 2, 4)
    bt.load_host(np.array([0, 2, 3], np.uint64), np.array([5, 5, 9], np.uint64), None, np.ones(2, np.float32))
    bt.localize()
    v = bt.get_key_view()
    bt.close()
    return {k: v[k] for k in ("BWD_SMALL", "BWD_MID", "HOT_SPLIT", "HOT_SPLIT_MIN")}


KW = dict(l1=0.01, l2=0.0, lr=0.1, seed=3)


def _load(bt, mb):
    bt.load_host(mb["offset"], mb["index"], mb["value"], mb["label"])


def localized(capi, ctx, oracle, mb, path, max_index=2 ** 64 - 1, stale_sizes=None):
    """the minibatch localized through `path`: (batch object, table of the probe or None, its bucket starts if designed)"""
    N, nrows = int(mb["offset"][-1]), len(mb["label"])
    primer = None
    if path == "stale":
        stale_sizes = stale_sizes or K.generic_stale_sizes(mb["lens"])
        primer = K.stale_primer(mb["lens"], stale_sizes, 17)
    bt = capi.Batch(ctx, max(nrows, len(primer["label"]) if primer else 0), N)
    tb, want_bstart = None, None
    bt.set_option("force_radix_sort", path == "radix")
    bt.set_option("force_sort_fallback", path == "fallback")
    if path == "host":
        loc = oracle.localize(mb["offset"], mb["index"], max_index)
        bt.load_localized_host(mb["offset"], loc["index"], mb["value"], mb["label"], loc["feaids"])
        return bt, tb, want_bstart
    if path == "stale":
        _load(bt, primer)
        bt.localize()
        want_bstart = np.concatenate([[0], np.cumsum(stale_sizes)])
    elif path == "stored":
        _load(bt, mb)
        bt.localize(max_index)
        want_bstart = "stored"
    _load(bt, mb)
    if path == "probe":
        tb = capi.Table(ctx, 1 << 15, V_dim=0, **KW)
        bt.localize(max_index, table=tb)
    else:
        bt.localize(max_index)
    return bt, tb, want_bstart


def view_and_check(oracle, bt, mb, path, bounds, want_bstart=None, max_index=2 ** 64 - 1, split="skip", split_entries=None):
    got = bt.get_key_view()
    ref = K.reference(mb["offset"], oracle.localize(mb["offset"], mb["index"], max_index)["index"], mb["value"], bounds)
    N = int(mb["offset"][-1])
    if path in ("radix", "host"):
        assert got["P"] == 0 and got["bstart"] is None and got["seg_nb"] == 1
    elif path is not None and N <= 65536:
        assert got["P"] == K.cold_buckets(N) and got["seg_nb"] == got["P"]
    if isinstance(want_bstart, str):
        want_bstart = K.stored_bstart(ref["s_row"], N, K.cold_buckets(N))
    if want_bstart is not None:     # the design holds: the buckets are cut where the case says they are
        assert np.array_equal(got["bstart"], want_bstart), "bucket starts of path %s" % path
        if path == "stale" and len(want_bstart) > 4:
            n_b = np.diff(want_bstart)
            assert (n_b == 0).sum() >= 2 and (N < 2400 or n_b.max() > K.LDS_CAP)
    K.check_key_view(got, ref, split=split, split_entries=split_entries)
    return got, ref


def run_case(capi, ctx, oracle, bounds, mb, path, **kw):
    """a fresh batch object, never stepped: its split list is empty"""
    kw.setdefault("split", "empty")
    bt, tb, want = localized(capi, ctx, oracle, mb, path, kw.get("max_index", 2 ** 64 - 1), kw.pop("stale_sizes", None))
    try:
        return view_and_check(oracle, bt, mb, path, bounds, want, **kw)
    finally:
        bt.close()
        if tb is not None:
            tb.close()


@gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("last", range(6))
def test_class_edges(capi, ctx, oracle, bounds, path, last):
    """segments of length 1, 2, BWD_SMALL, BWD_SMALL + 1, BWD_MID, BWD_MID + 1 in mixed order; each of them as the last key
    (the end of the minibatch closes it) and as the first"""
    for first in range(6):
        mb = K.batch_from_lens(K.class_edge_lens(bounds, first, last), 100 + 6 * last + first, binary=(first % 2 == 1))
        run_case(capi, ctx, oracle, bounds, mb, path)


@gpu
@pytest.mark.parametrize("path", PATHS)
def test_class_edges_lone_pair_after_a_hot_key(capi, ctx, oracle, bounds, path):
    mb = K.batch_from_lens(K.class_edge_lens(bounds, 2, 0, lone_tail=True), 7)
    run_case(capi, ctx, oracle, bounds, mb, path)


@gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("ending", ["inside_run", "single"])
def test_bucket_stitching(capi, ctx, oracle, bounds, path, ending):
    """runs that end on, begin on and straddle the cuts of 16 buckets, cover whole buckets (no head inside: cont = 1), and
    are still open where the minibatch ends; `stored` cuts exactly at the multiples of 192 (asserted through bstart)"""
    mb = K.batch_from_lens(K.stitch_layout(bounds, ending).lens, 41)
    got, _ = run_case(capi, ctx, oracle, bounds, mb, path)
    if path == "stored":
        assert np.array_equal(got["bstart"], K.stitch_layout(bounds, ending).cuts)


@gpu
@pytest.mark.parametrize("path", ["cold", "stored", "stale"])
@pytest.mark.parametrize("which", range(3))
def test_worst_legal_list_shape(capi, ctx, oracle, bounds, path, which):
    """every key exactly 2 / BWD_SMALL + 1 / BWD_MID + 1 times: as many entries per bucket as a list can get — where a bucket
    fills its slot range"""
    mb = K.batch_from_lens(worst_lens(bounds, which), 50 + which, binary=(which == 1))
    got, ref = run_case(capi, ctx, oracle, bounds, mb, path)
    name = ["few", "mid", "hot"][which]
    assert len(ref[name]) == ref["U"] and int(got[name]["desc"][:, 0].sum()) == ref["U"]


@gpu
@pytest.mark.parametrize("i", range(12))
def test_one_key_only(capi, ctx, oracle, bounds, i):
    """one key of N occurrences, a run across every bucket; after one training step the split list holds
    0, ..., 0, 5, 5, 6 parts with the expected contents"""
    N = ONE_KEY_N(bounds)[i]
    mb = K.batch_from_lens([N], 60 + i, nrows=max(1, N // 3))
    bt, _, _ = localized(capi, ctx, oracle, mb, "cold")
    tb = capi.Table(ctx, 1 << 10, V_dim=0, **KW)
    try:
        view_and_check(oracle, bt, mb, "cold", bounds, split="empty", split_entries=bt.split_entries())
        bt.sgd_step(tb, is_train=True, push_cnt=True)
        got, _ = view_and_check(oracle, bt, mb, "cold", bounds, split="listed", split_entries=bt.split_entries())
        hs, hsm = bounds["HOT_SPLIT"], bounds["HOT_SPLIT_MIN"]
        assert got["split_n"] == (0 if N <= hsm else -(-N // hs))
        if bounds == NOMINAL:
            assert got["split_n"] == ([0] * 8 + [0, 5, 5, 6])[i]
        tb.check()
    finally:
        bt.close()
        tb.close()


@gpu
def test_mixed_with_a_second_step(capi, ctx, oracle, bounds):
    """the mixed minibatch of test_split_list.py::test_boundaries_of_the_cut, stepped twice: the split list is emptied and
    refilled, not appended to — and reading the key view changes nothing: the steps of a batch object that was read give
    the logits and the model, bit for bit, of one that was not"""
    mb = K.batch_from_lens(MIXED(bounds), 71, special_values=False)
    mb["label"] = np.where(mb["label"] > 0, 1.0, 0.0).astype(np.float32)
    keys = oracle.localize(mb["offset"], mb["index"])["feaids"]
    out = []
    for read in (False, True):
        bt, _, _ = localized(capi, ctx, oracle, mb, "cold")
        tb = capi.Table(ctx, 1 << 10, V_dim=0, **KW)
        preds = []
        try:
            for step in range(2):
                if read:
                    view_and_check(oracle, bt, mb, "cold", bounds, split="empty" if step == 0 else "listed")
                bt.sgd_step(tb, is_train=True, push_cnt=(step == 0))
                preds.append(bt.pred())
                if read:
                    got, ref = view_and_check(oracle, bt, mb, "cold", bounds, split="listed", split_entries=bt.split_entries())
                    if bounds == NOMINAL:
                        assert got["split_n"] == 8 + 5
                else:
                    assert bt.split_entries() == len(K.reference(mb["offset"], mb["cidx"], mb["value"], bounds)["split"])
            tb.check()
            out.append((preds, tb.pull(keys)))
        finally:
            bt.close()
            tb.close()
    (p0, (v0, l0)), (p1, (v1, l1)) = out
    for a, b in zip(p0, p1):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "logits differ after get_key_view"
    assert np.array_equal(l0, l1) and np.array_equal(v0.view(np.uint32), v1.view(np.uint32)), "model differs after get_key_view"


@gpu
def test_chunk_carry_inside_a_bucket(capi, ctx, oracle, bounds):
    """under stale splitters a bucket of 800 pairs and one of 1 100 (the global-memory sort), empty buckets around them;
    a pair as 255 | 1, runs of 9 and 12 and a run of 300 across the 256-element chunks of emit"""
    L, sizes = K.chunk_carry_layout()
    mb = K.batch_from_lens(L.lens, 83)
    got, _ = run_case(capi, ctx, oracle, bounds, mb, "stale", stale_sizes=sizes)
    assert np.array_equal(np.diff(got["bstart"].astype(np.int64)), sizes)


_ROWS = {}


def rows_case(name, bounds):
    if name not in _ROWS:
        if name == "tb15":
            mb = ragged_rows_batch()
        elif name == "over_sample_sort":
            from difacto_amd import synth
            mb = synth.CriteoSynth(total_ids=3000000, seed=5).batch(18380)
            assert int(mb["offset"][-1]) > 716800
        else:
            mb = K.batch_from_lens(K.class_edge_lens(bounds, 4, 5) * 6, 91, one_row=True)
            assert len(mb["label"]) == 1
        _ROWS[name] = (mb, K.reference(mb["offset"], numpy_localize(mb), mb["value"], bounds))
    return _ROWS[name]


@gpu
@pytest.mark.parametrize("path", ["cold", "radix"])
@pytest.mark.parametrize("name", ["tb15", "over_sample_sort", "one_row"])
def test_row_reconstruction(capi, ctx, oracle, bounds, name, path):
    """s_row from the tag's low row bits and a search over the candidate rows: 15 row bits and two candidates among empty
    rows; the large size class (12 row bits, five candidates); one row holding everything"""
    mb, ref = rows_case(name, bounds)
    bt = capi.Batch(ctx, len(mb["label"]), int(mb["offset"][-1]))
    try:
        bt.set_option("force_radix_sort", path == "radix")
        _load(bt, mb)
        bt.localize()
        got = bt.get_key_view()
        assert (got["P"] > 0) == (path == "cold")
        K.check_key_view(got, ref, split="empty")
        assert np.array_equal(bt.get_localized()["index"], numpy_localize(mb))
    finally:
        bt.close()


@gpu
@pytest.mark.parametrize("path", ["cold", "stored", "fallback", "radix", "host"])
def test_s_val_specials(capi, ctx, oracle, bounds, path):
    """-0.0, the infinities, NaNs with payloads and denormals travel into s_val bit for bit"""
    mb = K.batch_from_lens(K.class_edge_lens(bounds, 1, 3) * 2, 97, special_values=True)
    bits = mb["value"].view(np.uint32)
    assert {0x80000000, 0x7F800000, 0x7FC01234, 0x00000001} <= set(bits.tolist())
    run_case(capi, ctx, oracle, bounds, mb, path)


@gpu
@pytest.mark.parametrize("path", ["cold", "stored", "fallback", "radix", "host", "probe"])
@pytest.mark.parametrize("max_index", [7, 1000])
def test_hashed_ids(capi, ctx, oracle, bounds, max_index, path):
    mb = hashed_batch()
    got, ref = run_case(capi, ctx, oracle, bounds, mb, path, max_index=max_index)
    assert ref["U"] <= max_index and (max_index != 7 or len(ref["hot"]) == 7)


@gpu
def test_prepare_cached(capi, ctx, oracle, bounds):
    """the count pass that gathers the rows out of a row buffer (the second call: the splitters are stored), compared after
    the step that consumes the preparation"""
    mb = K.batch_from_lens(K.stitch_layout(bounds, "single").lens + [bounds["HOT_SPLIT_MIN"] + 1], 103)
    mb["label"] = np.where(mb["label"] > 0, 1.0, 0.0).astype(np.float32)
    N, nrows = int(mb["offset"][-1]), len(mb["label"])
    rb = capi.RowBuf(ctx, nrows, N)
    bt = capi.Batch(ctx, nrows, N)
    tb = capi.Table(ctx, 1 << 15, V_dim=0, **KW)
    try:
        rb.load_host(mb["offset"], mb["index"], mb["value"])
        rb.set_labels(mb["label"])
        for rnd in range(2):
            bt.prepare_cached(tb, [(rb, np.arange(nrows))])
            bt.sgd_step(tb, is_train=True, push_cnt=(rnd == 0))
            got, _ = view_and_check(oracle, bt, mb, "cold", bounds, "stored" if rnd else None, split="listed",
                                    split_entries=bt.split_entries())
            assert got["split_n"] > 0
        tb.check()
    finally:
        for o in (bt, rb, tb):
            o.close()


@gpu
def test_single_queue(capi, oracle, bounds):
    """a single-queue context: the Localizer's stages of the minibatches prepared ahead ride in the launches of the steps
    before them; every minibatch is compared after its own step"""
    designs = [K.stitch_layout(bounds, "inside_run").lens, K.stitch_layout(bounds, "single").lens, K.chunk_carry_layout()[0].lens,
               [K.SMALL_AVG * 16 - 300, 300], K.class_edge_lens(bounds, 5, 5)]
    designs[4] = designs[4] * (16 * K.SMALL_AVG // sum(designs[4]))
    designs[4] = designs[4] + [1] * (16 * K.SMALL_AVG - sum(designs[4]))
    mbs = [K.batch_from_lens(lens, 110 + i, nrows=700) for i, lens in enumerate(designs)]
    assert {int(mb["offset"][-1]) for mb in mbs} == {16 * K.SMALL_AVG}
    for mb in mbs:
        mb["label"] = np.where(mb["label"] > 0, 1.0, 0.0).astype(np.float32)
    c = capi.Context(0)
    c.set_option("single_queue", 1)
    tb = capi.Table(c, 1 << 15, V_dim=0, **KW)
    bts = [capi.Batch(c, 700, 16 * K.SMALL_AVG) for _ in range(3)]
    nsteps = 11

    def prep(i):
        _load(bts[i % 3], mbs[i % len(mbs)])
        bts[i % 3].localize()

    try:
        prep(0)
        prep(1)
        for i in range(nsteps):
            if i + 2 < nsteps:
                prep(i + 2)
            bt, mb = bts[i % 3], mbs[i % len(mbs)]
            bt.sgd_step(tb, is_train=True, push_cnt=(i < len(mbs)))
            # (from the fourth step on not a first call of its batch object: the stages were noted and rode)
            view_and_check(oracle, bt, mb, "cold", bounds, split="listed", split_entries=bt.split_entries())
        tb.check()
    finally:
        for o in bts + [tb]:
            o.close()
        c.close()


@gpu
def test_refused_calls_leave_the_object_usable(capi, ctx, oracle, bounds):
    bt = capi.Batch(ctx, 8, 64)
    try:
        with pytest.raises(capi.DfhError):
            bt.get_key_view()                                   # nothing loaded, not localized
        mb = K.batch_from_lens([3, 1, bounds["BWD_SMALL"] + 1], 5)
        _load(bt, mb)
        with pytest.raises(capi.DfhError):
            bt.get_key_view()                                   # loaded, not localized
        assert capi.lib().dfh_batch_key_view_info(bt.h, None) != 0
        assert capi.lib().dfh_batch_key_view_info(None, None) != 0
        assert capi.lib().dfh_batch_get_key_view(*([None] * 12)) != 0
        bt.localize()
        assert capi.lib().dfh_batch_key_view_info(bt.h, None) != 0
        assert capi.lib().dfh_batch_get_key_view(bt.h, *([None] * 11)) == 0      # every array is optional
        view_and_check(oracle, bt, mb, "cold", bounds, split="empty")
    finally:
        bt.close()
