"""The device row store (dfh_rowstore, csrc/dfh_rowstore.hip) through ctypes: rows appended chunk by chunk into slabs in HBM, the
splitmix64 order over them, and blocks of that order gathered back to the host (dfh_rowstore_read) and into the record encoder
(dfh_crb_encode_rowstore).

The reference for everything is numpy on the appended arrays: the order is a stable argsort of the keys, a block is the
gather of its rows, and its record is what dfh_crb_encode_host writes for that gather, byte for byte."""
import threading

import numpy as np
import pytest

from test_crb_encode import built, check_record, fields_of, host_parse, ing, ref_crb  # noqa: F401  (fixtures)
from test_text_parse import _regular_case

SLAB = 4096   # 512 ids per slab, 256 rows per segment of row records
M64 = (1 << 64) - 1
ERR_ARG, ERR_STATE = 1, 4   # DFH_ERR_ARG, DFH_ERR_STATE of include/difacto_hip.h


def splitmix_keys(n, seed):
    """key(r) = output r of splitmix64(seed), r = 0 .. n - 1, in Python integers"""
    out = np.zeros(n, np.uint64)
    for r in range(n):
        z = (seed + (r + 1) * 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        out[r] = z ^ (z >> 31)
    return out


def want_order(n, shuffle, seed):
    return np.argsort(splitmix_keys(n, seed), kind="stable").astype(np.uint32) if shuffle else np.arange(n, dtype=np.uint32)


class Rows:
    """the appended rows on the host: what numpy gathers from"""

    def __init__(self):
        self.lens, self.label, self.ids, self.val, self.wgt = [], [], [], [], []

    def add(self, off, lab, idx, val=None, wgt=None):
        off = np.asarray(off, np.int64) - int(off[0])
        for r in range(len(off) - 1):
            a, b = off[r], off[r + 1]
            self.lens.append(b - a)
            self.label.append(lab[r])
            self.ids.append(np.asarray(idx[a:b], np.uint64))
            self.val.append(np.ones(b - a, np.float32) if val is None else np.asarray(val[a:b], np.float32))
            self.wgt.append(None if wgt is None else wgt[r])

    def __len__(self):
        return len(self.lens)

    def block(self, rows):
        """-> offset from 0, label, index, value, weight | None of these rows in this order"""
        off = np.zeros(len(rows) + 1, np.uint64)
        off[1:] = np.cumsum([self.lens[r] for r in rows])
        lab = np.array([self.label[r] for r in rows], np.float32)
        idx = np.concatenate([self.ids[r] for r in rows] + [np.zeros(0, np.uint64)])
        val = np.concatenate([self.val[r] for r in rows] + [np.zeros(0, np.float32)])
        wgt = None if not rows or self.wgt[rows[0]] is None else np.array([self.wgt[r] for r in rows], np.float32)
        return off, lab, idx, val, wgt


def designed_chunks(weighted=False):
    """7 chunks, 2 003 rows of 0, 1, 39 and 300 ids and one of 600 (more than a slab holds); ids with their high bits set; chunks 2
    and 5 carry real values, chunk 3 values that are all 1.0f, the others none; a chunk fills many slabs"""
    rng = np.random.default_rng(20)
    sizes = [1, 350, 300, 2, 640, 400, 310]
    chunks = []
    for k, nrows in enumerate(sizes):
        lens = rng.choice([0, 1, 39, 300], size=nrows, p=[0.15, 0.2, 0.55, 0.1])
        if k == 4:
            lens[17] = 600
            lens[18:22] = 0
        if k == 0:
            lens[:] = 39
        off = np.zeros(nrows + 1, np.uint64)
        off[1:] = np.cumsum(lens)
        off += np.uint64((0, 0, 77, 0, 5, 0, 1 << 33)[k])   # a chunk's offsets need not start at 0
        nnz = int(off[-1] - off[0])
        idx = rng.integers(0, 1 << 63, size=nnz, dtype=np.uint64) | np.uint64(1 << 63)
        lab = rng.integers(0, 2, size=nrows).astype(np.float32)
        val = None
        if k in (2, 5):
            val = rng.normal(size=nnz).astype(np.float32)
        elif k == 3:
            val = np.ones(nnz, np.float32)
        wgt = rng.random(nrows).astype(np.float32) if weighted else None
        chunks.append((off, lab, idx, val, wgt))
    return chunks


def fill(capi, ctx, chunks, slab=SLAB):
    st, rows = capi.RowStore(ctx, slab), Rows()
    for c in chunks:
        st.append_host(*c)
        rows.add(*c)
    return st, rows


@pytest.fixture(scope="module")
def dev(built):  # noqa: F811
    from difacto_amd import capi
    ctx = capi.Context(0)
    encs = [capi.CrbEncoder(ctx) for _ in range(3)]
    yield capi, ctx, encs
    for e in encs:
        e.close()
    ctx.close()


@pytest.fixture(scope="module")
def designed(dev):
    """the designed store, ordered with seed 7, and its rows on the host"""
    capi, ctx, _ = dev
    st, rows = fill(capi, ctx, designed_chunks())
    st.order(1, 7)
    yield st, rows, [int(r) for r in want_order(len(rows), 1, 7)]
    st.close()


def ranges(n):
    return [(0, n), (0, 1), (n - 1, 1), (17, 64), (63, 130), (n, 0)]


RANGE_NAMES = ["all", "first_row", "last_row", "17_64", "63_130", "none_at_the_end"]


def test_the_symbols_are_declared():
    from difacto_amd import capi
    for name in ("dfh_rowstore_create", "dfh_rowstore_destroy", "dfh_rowstore_append_host", "dfh_rowstore_append_textchunk",
                 "dfh_rowstore_shape", "dfh_rowstore_order", "dfh_rowstore_get_order", "dfh_rowstore_read", "dfh_crb_encode_rowstore"):
        assert name in capi.SYMBOLS


@pytest.mark.gpu
def test_shape_of_the_designed_store(designed):
    st, rows, _ = designed
    s = st.shape()
    assert s["nrows"] == len(rows) == 2003 and s["nnz"] == sum(rows.lens) and s["has_value"] and not s["has_weight"]
    assert max(rows.lens) == 600 and {0, 1, 39, 300} <= set(rows.lens)
    # ids alone are nnz * 8 bytes in slabs of 4 096: far more slabs than chunks, and a row of 600 ids has its own
    assert s["device_bytes"] >= s["nnz"] * 8 + s["nrows"] * 16
    assert s["nnz"] * 8 // SLAB > 50


@pytest.mark.gpu
def test_order(designed):
    st, rows, order7 = designed
    n = len(rows)
    try:
        for seed in (0, 1, M64):
            st.order(1, seed)
            got = st.get_order()
            assert got.dtype == np.uint32 and np.array_equal(got, want_order(n, 1, seed)), seed
            assert np.array_equal(np.sort(got), np.arange(n))
        assert not np.array_equal(want_order(n, 1, 0), want_order(n, 1, 1))
        st.order(0, 5)
        assert np.array_equal(st.get_order(), np.arange(n))
    finally:
        st.order(1, 7)   # what the other tests of the module read
    assert np.array_equal(st.get_order(), np.array(order7, np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(6), ids=RANGE_NAMES)
def test_read(designed, which):
    st, rows, order = designed
    first, count = ranges(len(rows))[which]
    off, lab, idx, val, wgt = st.read(first, count)
    w_off, w_lab, w_idx, w_val, _ = rows.block(order[first:first + count])
    assert off.dtype == np.uint64 and np.array_equal(off, w_off)
    assert lab.tobytes() == w_lab.tobytes()
    assert np.array_equal(idx, w_idx)
    assert val.tobytes() == w_val.tobytes()
    assert wgt is None


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(6), ids=RANGE_NAMES)
def test_records(dev, designed, ing, ref_crb, tmp_path, which):  # noqa: F811
    _, _, encs = dev
    st, rows, order = designed
    first, count = ranges(len(rows))[which]
    w_off, w_lab, w_idx, w_val, _ = rows.block(order[first:first + count])
    rec = encs[0].encode_rowstore(st, first, count)
    assert rec == encs[1].encode_host(w_off, w_lab, w_idx, w_val)
    check_record(ing, ref_crb, tmp_path, rec, w_off, w_lab, w_idx, w_val)
    assert encs[0].encode_rowstore(st, first, count) == rec


@pytest.mark.gpu
def test_three_encoders_on_one_store(dev, designed):
    """three threads, each with its own encoder, cut the order into records of 97 rows between them"""
    _, _, encs = dev
    st, rows, order = designed
    n = len(rows)
    blocks = [(at, min(97, n - at)) for at in range(0, n, 97)]
    got, errors = {}, []

    def work(k):
        try:
            for b in blocks[k::3]:
                got[b] = encs[k].encode_rowstore(st, *b)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(got) == len(blocks) == 21
    for first, count in blocks:
        w_off, w_lab, w_idx, w_val, _ = rows.block(order[first:first + count])
        assert got[first, count] == encs[0].encode_host(w_off, w_lab, w_idx, w_val), (first, count)


@pytest.mark.gpu
def test_values_all_ones_are_dropped_per_block(dev, ing):  # noqa: F811
    """rows without values, rows whose values are all 1.0f and one row with a single 0.5, in file order: the block that holds the
    0.5 keeps its value array, every other block has none"""
    capi, ctx, encs = dev
    rng = np.random.default_rng(4)

    def chunk(nrows, valued):
        off = np.arange(nrows + 1, dtype=np.uint64) * np.uint64(39)
        idx = rng.integers(0, M64, size=39 * nrows, dtype=np.uint64)
        return off, rng.integers(0, 2, size=nrows).astype(np.float32), idx, (np.ones(39 * nrows, np.float32) if valued else None), None

    chunks = [chunk(100, False), chunk(100, True), chunk(100, True), chunk(100, False)]
    chunks[2][3][39 * 50 + 7] = 0.5   # row 250
    st, rows = fill(capi, ctx, chunks)
    try:
        assert st.shape()["has_value"]
        st.order(0)
        for first, count, kept in ((0, 100, False), (100, 100, False), (200, 100, True), (250, 1, True), (251, 149, False), (0, 250, False),
                                   (0, 400, True), (300, 100, False)):
            rec = encs[0].encode_rowstore(st, first, count)
            _, f = fields_of(ing, rec)
            assert (f["value"] is not None) == kept, (first, count)
            w_off, w_lab, w_idx, w_val, _ = rows.block(list(range(first, first + count)))
            assert rec == encs[1].encode_host(w_off, w_lab, w_idx, w_val)
            assert st.read(first, count)[3].tobytes() == w_val.tobytes()
    finally:
        st.close()


@pytest.mark.gpu
def test_a_store_without_values(dev, ing):  # noqa: F811
    capi, ctx, encs = dev
    chunks = [c[:3] + (None, None) for c in designed_chunks()]
    st, rows = fill(capi, ctx, chunks)
    try:
        assert not st.shape()["has_value"]
        st.order(1, 3)
        order = [int(r) for r in want_order(len(rows), 1, 3)]
        w_off, w_lab, w_idx, w_val, _ = rows.block(order[63:193])
        rec = encs[0].encode_rowstore(st, 63, 130)
        assert rec == encs[1].encode_host(w_off, w_lab, w_idx) and fields_of(ing, rec)[1]["value"] is None
        got = st.read(63, 130)
        assert np.array_equal(got[2], w_idx) and np.all(got[3] == 1) and len(got[3]) == len(w_idx)
    finally:
        st.close()


@pytest.mark.gpu
def test_weights_in_every_chunk_or_in_none(dev, ing, ref_crb, tmp_path):  # noqa: F811
    capi, ctx, encs = dev
    chunks = designed_chunks(weighted=True)
    st, rows = fill(capi, ctx, chunks)
    try:
        assert st.shape()["has_weight"]
        st.order(1, 11)
        order = [int(r) for r in want_order(len(rows), 1, 11)]
        for first, count in ((0, len(rows)), (17, 64), (len(rows), 0)):
            w = rows.block(order[first:first + count])
            rec = encs[0].encode_rowstore(st, first, count)
            assert rec == encs[1].encode_host(*w)
            check_record(ing, ref_crb, tmp_path, rec, *w)
            got = st.read(first, count)
            assert (got[4].tobytes() == w[4].tobytes()) if count else len(got[4]) == 0
        off, lab, idx, val, _ = chunks[1]
        with pytest.raises(capi.DfhError, match="weights") as e:
            st.append_host(off, lab, idx, val, None)
        assert e.value.code == ERR_ARG
        assert st.shape()["nrows"] == len(rows)
    finally:
        st.close()
    st = capi.RowStore(ctx, SLAB)
    try:
        st.append_host(*chunks[1][:4], None)
        with pytest.raises(capi.DfhError, match="weights"):
            st.append_host(*chunks[2])
    finally:
        st.close()


@pytest.mark.gpu
def test_text_chunks_device_to_device(dev, ing):  # noqa: F811
    """the same criteo text through append_textchunk (its ids never leave HBM) and through append_host of the host parse"""
    capi, ctx, encs = dev
    tc = capi.TextChunk(ctx, 1 << 12)
    a, b = capi.RowStore(ctx, SLAB), capi.RowStore(ctx, SLAB)
    rows = Rows()
    try:
        for name in ("rows_65", "empty_rows", "rows_1", "longest_row", "rows_5000", "only_empty_rows", "int_lengths"):
            text, train = _regular_case(name, np.random.default_rng(sum(name.encode())))
            assert tc.parse_criteo(text, is_train=train) is not None, name
            a.append_textchunk(tc)
            off, lab, idx = host_parse(ing, text, train)
            b.append_host(off, lab, idx)
            rows.add(off, lab, idx)
        n = len(rows)
        assert a.shape() == b.shape() and a.shape()["nrows"] == n > 5000 and not a.shape()["has_value"]
        a.order(1, 99)
        b.order(1, 99)
        order = [int(r) for r in want_order(n, 1, 99)]
        assert np.array_equal(a.get_order(), b.get_order()) and np.array_equal(a.get_order(), np.array(order, np.uint32))
        for first, count in ranges(n):
            w_off, w_lab, w_idx, _, _ = rows.block(order[first:first + count])
            ra, rb = a.read(first, count), b.read(first, count)
            for x, y, w in zip(ra[:3], rb[:3], (w_off, w_lab, w_idx)):
                assert x.tobytes() == y.tobytes() == w.tobytes()
            rec = encs[0].encode_rowstore(a, first, count)
            assert rec == encs[1].encode_rowstore(b, first, count) == encs[2].encode_host(w_off, w_lab, w_idx)
    finally:
        a.close()
        b.close()
        tc.close()


@pytest.mark.gpu
def test_the_cut_into_appends_does_not_matter(dev, designed):
    """the designed rows appended row by row in part, in two halves in part, into slabs of another size: the same order, reads
    and records; the same appends twice: the same again"""
    capi, ctx, encs = dev
    st, rows, order = designed
    n = len(rows)
    cuts = [0, 1, 2, 3, 350, 351, 1000, 1001, 1002, 1650, n]

    def recut(slab):
        other = capi.RowStore(ctx, slab)
        for a, b in zip(cuts, cuts[1:]):
            off, lab, idx, val, _ = rows.block(list(range(a, b)))
            other.append_host(off + np.uint64(a), lab, idx, val)
        other.order(1, 7)
        return other

    others = [recut(SLAB), recut(SLAB), recut(1 << 16)]
    try:
        for o in others:
            assert o.shape()["nrows"] == n and np.array_equal(o.get_order(), st.get_order())
        for first, count in ranges(n):
            rec = encs[0].encode_rowstore(st, first, count)
            for o in others:
                assert encs[1].encode_rowstore(o, first, count) == rec
                for x, y in zip(o.read(first, count)[:4], st.read(first, count)[:4]):
                    assert x.tobytes() == y.tobytes()
    finally:
        for o in others:
            o.close()


@pytest.mark.gpu
def test_errors(dev, designed):
    capi, ctx, encs = dev
    _, rows, _ = designed
    st = capi.RowStore(ctx, SLAB)
    try:
        off, lab, idx, val, _ = rows.block(list(range(100)))
        st.append_host(off, lab, idx, val)
        with pytest.raises(capi.DfhError, match="no order") as e_enc:
            encs[0].encode_rowstore(st, 0, 10)
        with pytest.raises(capi.DfhError, match="no order") as e_read:
            st.read(0, 10)
        with pytest.raises(capi.DfhError, match="no order"):
            st.get_order()
        assert e_enc.value.code == e_read.value.code == ERR_STATE
        st.order(1, 1)
        assert len(encs[0].encode_rowstore(st, 90, 10)) > 0
        for first, count in ((91, 10), (101, 0), (0, 101), (M64, 2)):
            with pytest.raises(capi.DfhError, match="of an order of 100 rows") as e:
                encs[0].encode_rowstore(st, first, count)
            assert e.value.code == ERR_ARG
            with pytest.raises(capi.DfhError, match="of an order of 100 rows") as e:
                st.read(first, count)
            assert e.value.code == ERR_ARG
        st.append_host(off, lab, idx, val)   # an append drops the order
        with pytest.raises(capi.DfhError, match="no order"):
            encs[0].encode_rowstore(st, 0, 10)
        st.order(0)
        assert st.shape()["nrows"] == 200 and np.array_equal(st.read(100, 100)[2], idx)
    finally:
        st.close()
