"""rec_decode = device, the C ABI: one CompressedRowBlock record -> a chunk whose ids stay in HBM (dfh_textchunk_decode_crb,
csrc/dfh_lz4dec.hip).

A regular record — ids only, as criteo records are — gives back exactly the arrays that went in; every other record is reported
as not regular (DFH_OK, nothing else said) and is left to the host decoder.  Records come from the product's encoder
(capi.CrbEncoder.encode_host), from oracle.ingest.write_crb_record (liblz4's bytes) where liblz4 loads, and from the reference's
CompressedRowBlock::Compress (tests/golden/ref_ingest.npz).  Downstream: the decoded chunk feeds dfh_rowbuf_load_slices and
dfh_crb_encode_textchunk as a device-parsed chunk of text does."""
import os
import struct

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_INGEST = os.path.join(ROOT, "tests", "golden", "ref_ingest.npz")
CRB_MAGIC = 1196140743


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


@pytest.fixture(scope="module")
def dev(built):
    """a context, one chunk object reused by every case (its arrays grow and are reused, as in the reader's pool), an encoder"""
    from difacto_amd import capi
    ctx = capi.Context(0)
    tc = capi.TextChunk(ctx, 1)
    enc = capi.CrbEncoder(ctx)
    yield capi, ctx, tc, enc
    enc.close()
    tc.close()
    ctx.close()


def writers(enc):
    """name -> f(offset, label or None, index, value, weight) -> record"""
    from oracle import ingest as oi
    out = {"device encoder": lambda off, lab, idx, val=None, wgt=None: enc.encode_host(off, lab, idx, val, wgt)}
    try:
        oi.liblz4()
        out["liblz4"] = lambda off, lab, idx, val=None, wgt=None: oi.write_crb_record(off, lab, idx, val, wgt)
    except OSError:
        pass
    return out


def rows(seed, lens, first=0):
    rng = np.random.default_rng(seed)
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    nnz = int(off[-1])
    # criteo-like: a hash in the high bits, the field's slot in the low 12
    idx = (rng.integers(0, 1 << 20, size=nnz, dtype=np.uint64) << np.uint64(12)) | (np.arange(nnz, dtype=np.uint64) % np.uint64(39))
    lab = (rng.random(len(lens)) < 0.3).astype(np.float32)
    return off + np.uint64(first), lab, idx


def decoded_equals(tc, rec, off, lab, idx):
    r = tc.decode_crb(rec)
    assert r is not None, "a regular record was not taken"
    d_off, d_lab, nnz = r
    assert d_off.dtype == np.uint32 and np.array_equal(d_off, (off - off[0]).astype(np.uint32))
    assert d_lab.tobytes() == np.asarray(lab, np.float32).tobytes()
    assert nnz == len(idx) and np.array_equal(tc.ids(nnz), idx)


SHAPES = {
    "1 row": ([5], 0),
    "3 rows, the middle one empty": ([4, 0, 7], 0),
    "257 rows of 39 ids": ([39] * 257, 0),
    "offset[0] = 1000": ([3, 9, 1, 39, 12], 1000),
    "12 000 rows": (None, 0),     # ids of 3.5 MB: hundreds of tiles, after which the small shapes reuse the grown arrays
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["12 000 rows", "1 row", "3 rows, the middle one empty", "257 rows of 39 ids", "offset[0] = 1000"])
def test_regular_records(dev, shape):
    capi, ctx, tc, enc = dev
    lens, first = SHAPES[shape]
    if lens is None:
        lens = np.random.default_rng(1).integers(20, 40, size=12000)
    off, lab, idx = rows(len(lens), lens, first)
    for name, write in writers(enc).items():
        decoded_equals(tc, write(off, lab, idx), off, lab, idx)
        # values that are all 1.0f are dropped by both writers: still ids only
        decoded_equals(tc, write(off, lab, idx, np.ones(len(idx), np.float32)), off, lab, idx)


@pytest.mark.gpu
def test_a_record_without_a_label_array(dev):
    capi, ctx, tc, enc = dev
    off, lab, idx = rows(3, [39] * 100)
    rec = enc.encode_host(off, lab, idx)
    # cut the label block out: {magic, 8, nrows}, int32 size, block, ...
    size = struct.unpack_from("<i", rec, 12)[0]
    assert size > 0
    rec = rec[:12] + struct.pack("<i", 0) + rec[16 + size:]
    decoded_equals(tc, rec, off, np.zeros(100, np.float32), idx)


def _golden():
    g = np.load(GOLDEN_INGEST)
    i = 0
    while "crb_rec_%d" % i in g:
        blk = {k: (g["crb_%d_%s" % (i, k)] if "crb_%d_%s" % (i, k) in g else None) for k in ("offset", "label", "index", "value", "weight")}
        yield g["crb_rec_%d" % i].tobytes(), blk
        i += 1


@pytest.mark.gpu
def test_the_references_records(dev):
    """regular where they have neither values (that are not all 1) nor weights and hold at least one row and one nonzero"""
    capi, ctx, tc, enc = dev
    seen = {True: 0, False: 0}
    for rec, b in _golden():
        off = b["offset"].astype(np.uint64)
        nrows, nnz = len(off) - 1, int(off[-1] - off[0])
        ids_only = (b["value"] is None or bool(np.all(b["value"] == 1))) and b["weight"] is None
        regular = ids_only and nrows >= 1 and nnz >= 1
        seen[regular] += 1
        if regular:
            lab = b["label"] if b["label"] is not None else np.zeros(nrows, np.float32)
            decoded_equals(tc, rec, off, lab, b["index"].astype(np.uint64))
        else:
            assert tc.decode_crb(rec) is None
    assert seen[True] >= 1 and seen[False] >= 1


@pytest.mark.gpu
def test_records_with_values_or_weights_are_left_to_the_host(dev):
    capi, ctx, tc, enc = dev
    off, lab, idx = rows(5, [7, 3, 39, 1])
    val = np.ones(len(idx), np.float32)
    val[11] = 0.5
    wgt = np.full(4, 2.0, np.float32)
    for name, write in writers(enc).items():
        assert tc.decode_crb(write(off, lab, idx, val)) is None
        assert tc.decode_crb(write(off, lab, idx, None, wgt)) is None
        assert tc.decode_crb(write(off, lab, idx, val, wgt)) is None
        decoded_equals(tc, write(off, lab, idx), off, lab, idx)   # (and the object is fine afterwards)


def _blocks(rec):
    """-> header ints and the five (size, bytes) of a record"""
    head = struct.unpack_from("<iii", rec, 0)
    cur, out = 12, []
    for _ in range(5):
        size = struct.unpack_from("<i", rec, cur)[0]
        cur += 4
        out.append(rec[cur:cur + max(size, 0)])
        cur += max(size, 0)
    assert cur == len(rec)
    return head, out


def _record(head, blocks):
    return struct.pack("<iii", *head) + b"".join(struct.pack("<i", len(b)) + b for b in blocks)


@pytest.mark.gpu
def test_malformed_records(dev):
    """each is DFH_OK with regular = 0 (decode_crb raises on any other return code)"""
    capi, ctx, tc, enc = dev
    off, lab, idx = rows(7, [39] * 50)
    good = enc.encode_host(off, lab, idx)
    head, blocks = _blocks(good)
    assert head == (CRB_MAGIC, 8, 50) and _record(head, blocks) == good
    decoded_equals(tc, good, off, lab, idx)
    assert tc.decode_crb(_record((CRB_MAGIC + 1, 8, 50), blocks)) is None            # wrong magic
    assert tc.decode_crb(_record((CRB_MAGIC, 4, 50), blocks)) is None                # index type 4
    assert tc.decode_crb(_record((CRB_MAGIC, 8, -50), blocks)) is None               # negative nrows
    assert tc.decode_crb(_record((CRB_MAGIC, 8, 0), blocks)) is None                 # no rows
    assert tc.decode_crb(_record((CRB_MAGIC, 8, 49), blocks)) is None                # nrows that the arrays do not have
    assert tc.decode_crb(_record((CRB_MAGIC, 8, 51), blocks)) is None
    # a decreasing offset pair
    bad = off.copy()
    bad[20], bad[21] = bad[21], bad[20]
    assert tc.decode_crb(_record(head, [blocks[0], capi.lz4_compress(ctx, bad.tobytes())] + blocks[2:])) is None
    # offsets that span more than the ids there are, and fewer
    for last in (int(off[-1]) + 1, int(off[-1]) - 1):
        bad = off.copy()
        bad[-1] = last
        assert tc.decode_crb(_record(head, [blocks[0], capi.lz4_compress(ctx, bad.tobytes())] + blocks[2:])) is None
    # an index block that inflates to 8 nnz - 8 bytes, and one of 8 nnz + 4
    assert tc.decode_crb(_record(head, blocks[:2] + [capi.lz4_compress(ctx, idx[:-1].tobytes())] + blocks[3:])) is None
    assert tc.decode_crb(_record(head, blocks[:2] + [capi.lz4_compress(ctx, idx.tobytes() + b"abcd")] + blocks[3:])) is None
    # a label block of the wrong size; blocks that are no LZ4 blocks
    assert tc.decode_crb(_record(head, [capi.lz4_compress(ctx, lab[:-1].tobytes())] + blocks[1:])) is None
    assert tc.decode_crb(_record(head, blocks[:2] + [blocks[2][:-7]] + blocks[3:])) is None
    assert tc.decode_crb(_record(head, [blocks[0], blocks[1][:-1]] + blocks[2:])) is None
    # no offsets, no ids
    assert tc.decode_crb(_record(head, [blocks[0], b""] + blocks[2:])) is None
    assert tc.decode_crb(_record(head, blocks[:2] + [b""] + blocks[3:])) is None
    # a record cut at each header word, inside a block, and before the last size word
    sizes = [12 + sum(4 + len(b) for b in blocks[:k]) for k in range(6)]
    for cut in [0, 3, 4, 8, 11, 12, 15] + [s + 4 for s in sizes[:4]] + [sizes[1] + 9, sizes[3] - 5, len(good) - 4, len(good) - 1]:
        assert tc.decode_crb(good[:cut]) is None, cut
    decoded_equals(tc, good, off, lab, idx)
    decoded_equals(tc, good + b"trailing bytes are ignored, as on the host", off, lab, idx)


@pytest.mark.gpu
def test_downstream_calls_take_the_decoded_chunk(dev):
    """dfh_crb_encode_textchunk of the decoded chunk is byte for byte dfh_crb_encode_host of the same rows, and
    dfh_rowbuf_load_slices fills a buffer whose gathered minibatches equal those of dfh_rowbuf_load_host"""
    capi, ctx, tc, enc = dev
    lens = np.random.default_rng(9).integers(0, 40, size=700)
    off, lab, idx = rows(9, lens, first=64)
    rec = enc.encode_host(off, lab, idx)
    decoded_equals(tc, rec, off, lab, idx)
    off0 = off - off[0]
    assert enc.encode_textchunk(tc) == enc.encode_host(off0, lab, idx)
    nrows, nnz = len(lens), len(idx)
    rb_ref, rb_dev = capi.RowBuf(ctx, nrows, nnz), capi.RowBuf(ctx, nrows, nnz)
    rb_ref.load_host(off0, idx, None)
    rb_dev.load_slices(off0, [(tc, 0, nnz)])
    ctx.set_pipeline(1)
    rng = np.random.default_rng(10)
    out = []
    for rb in (rb_ref, rb_dev):
        rb.set_labels(lab)
        bt = capi.Batch(ctx, nrows, max(nnz, 1))
        res = []
        for pick in (rng.permutation(nrows)[:257], np.arange(nrows)):
            pick = pick.astype(np.uint32)
            o = np.zeros(len(pick) + 1, np.uint64)
            o[1:] = np.cumsum(np.diff(off0.astype(np.int64))[pick])
            bt.gather_rows(o, lab[pick], [(rb, pick)])
            bt.localize()
            loc = bt.get_localized()
            res.append((loc["feaids"].tobytes(), loc["index"].tobytes(), loc["feacnt"].tobytes()))
        out.append(res)
        bt.close()
        rng = np.random.default_rng(10)
    assert out[0] == out[1]
    rb_ref.close()
    rb_dev.close()
