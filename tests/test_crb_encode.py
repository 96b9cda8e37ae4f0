"""CompressedRowBlock records written on the device (dfh_crb_encode_host / dfh_crb_encode_textchunk, csrc/dfh_lz4enc.hip).

A record decodes to the arrays that went in, bit for bit: through the product's reader (a one-record file written with
oracle.ingest.write_recordio, read with ingest_read format = rec, and DecompressRowBlock's own view through the same library)
and, where oracle/_ref was built with its data-format half, through the reference's CompressedRowBlock::Decompress.  The
record of a regular criteo chunk whose ids never left HBM equals the record of the host parser's arrays byte for byte."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from test_text_parse import _regular_case

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
def ing(built):
    L = C.CDLL(os.path.join(built, "libdifacto_ingest.so"))
    L.ingest_lz4_decompress.restype = C.c_long
    L.ingest_lz4_decompress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.ingest_read.restype = C.c_long
    L.ingest_read.argtypes = [C.c_char_p, C.c_char_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_size_t, C.c_size_t,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_long)]
    L.ingest_parse_criteo.restype = C.c_long
    L.ingest_parse_criteo.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def dev(built):
    """a context, ONE encoder and one text chunk object for every case: their arrays grow, and are reused by smaller blocks"""
    from difacto_amd import capi
    ctx = capi.Context(0)
    enc = capi.CrbEncoder(ctx)
    tc = capi.TextChunk(ctx, 1 << 12)
    yield capi, ctx, enc, tc
    tc.close()
    enc.close()
    ctx.close()


@pytest.fixture(scope="module")
def ref_crb():
    """the reference's own Decompress where oracle/_ref is built with its data-format half, else None"""
    from oracle import bindings
    if not bindings.have_ref():
        return None
    R = bindings.Ref()
    return R if R.has_ingest else None


def fields_of(ing, rec):
    """the record taken apart by its layout: (nrows, {name: bytes | None}), every block inflated by the product's decoder"""
    magic, isize, nrows = struct.unpack_from("<iii", rec, 0)
    assert magic == CRB_MAGIC and isize == 8 and nrows >= 0
    at, out = 12, {}
    for name, per in (("label", 4), ("offset", 8), ("index", 8), ("value", 4), ("weight", 4)):
        size, = struct.unpack_from("<i", rec, at)
        at += 4
        if size == 0:
            out[name] = None
            continue
        assert size > 0
        out[name] = (rec[at:at + size], per)
        at += size
    assert at == len(rec)
    off = _inflate(ing, out["offset"][0], (nrows + 1) * 8)
    nnz = int(np.frombuffer(off, np.uint64)[-1] - np.frombuffer(off, np.uint64)[0])
    res = {}
    for name, count in (("label", nrows), ("offset", nrows + 1), ("index", nnz), ("value", nnz), ("weight", nrows)):
        res[name] = None if out[name] is None else _inflate(ing, out[name][0], count * out[name][1])
    return nrows, res


def _inflate(ing, block, n):
    dst = C.create_string_buffer(n + 1)
    assert ing.ingest_lz4_decompress(block, len(block), dst, n) == n
    return dst.raw[:n]


def read_rec(ing, path):
    cap_rows, cap_nnz = 100000, 1000000
    off = np.zeros(cap_rows + 1, np.uint64)
    lab = np.zeros(cap_rows, np.float32)
    idx = np.zeros(cap_nnz, np.uint64)
    val = np.zeros(cap_nnz, np.float32)
    hv, nb = C.c_int(0), C.c_long(0)
    n = ing.ingest_read(str(path).encode(), b"rec", 0, 1, 64, 0, 1.0, cap_rows, cap_nnz, off.ctypes.data, lab.ctypes.data, idx.ctypes.data,
                        val.ctypes.data, C.byref(hv), C.byref(nb))
    assert n >= 0
    nnz = int(off[n])
    return off[:n + 1], lab[:n], idx[:nnz], val[:nnz], bool(hv.value)


def check_record(ing, ref_crb, tmp_path, rec, offset, label, index, value=None, weight=None):
    from oracle import ingest as oi
    offset = np.asarray(offset, np.uint64)
    label = np.asarray(label, np.float32)
    index = np.asarray(index, np.uint64)
    nrows = len(offset) - 1
    binary = value is None or bool(np.all(np.asarray(value) == 1))
    # the layout, field by field
    n, f = fields_of(ing, rec)
    assert n == nrows
    assert (f["label"] is None and nrows == 0) or f["label"] == label.tobytes()
    assert f["offset"] == offset.tobytes()                       # as given, offset[0] included
    assert (f["index"] is None and len(index) == 0) or f["index"] == index.tobytes()
    assert f["value"] is None if binary else f["value"] == np.asarray(value, np.float32).tobytes()
    assert f["weight"] is None if weight is None or nrows == 0 else f["weight"] == np.asarray(weight, np.float32).tobytes()
    # the product's reader
    if nrows:
        path = tmp_path / "one.rec"
        path.write_bytes(oi.write_recordio([rec]))
        off, lab, idx, val, has_value = read_rec(ing, path)
        assert off.tobytes() == (offset - offset[0]).tobytes() and lab.tobytes() == label.tobytes() and idx.tobytes() == index.tobytes()
        assert has_value == (not binary)
        assert val.tobytes() == (np.ones(len(index), np.float32) if binary else np.asarray(value, np.float32)).tobytes()
    # the reference's Decompress
    if ref_crb is not None and nrows:
        d = ref_crb.crb_decompress(rec)
        assert np.array_equal(d["offset"], offset) and d["label"].tobytes() == label.tobytes() and np.array_equal(d["index"], index)
        assert (d["value"] is None) == binary and (binary or d["value"].tobytes() == np.asarray(value, np.float32).tobytes())
        assert (d["weight"] is None) == (weight is None) and (weight is None or d["weight"].tobytes() == np.asarray(weight, np.float32).tobytes())


def block(rng, lens, first=0, valued=None, weighted=False):
    lens = np.asarray(lens, np.int64)
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    nnz = int(off[-1])
    off += np.uint64(first)
    idx = rng.integers(0, 2 ** 64 - 1, size=nnz, dtype=np.uint64)
    lab = rng.integers(0, 2, size=len(lens)).astype(np.float32)
    val = None
    if valued == "ones":
        val = np.ones(nnz, np.float32)
    elif valued == "one_differs":
        val = np.ones(nnz, np.float32)
        val[nnz // 2] = np.float32(1.0000001)
    elif valued == "real":
        val = rng.normal(size=nnz).astype(np.float32)
    wgt = rng.random(len(lens)).astype(np.float32) if weighted else None
    return off, lab, idx, val, wgt


SHAPES = {
    "one_row": dict(lens=[7]),
    "one_empty_row": dict(lens=[0]),
    "empty_rows_first_last_and_in_a_row": dict(lens=[0, 0, 5, 3, 0, 0, 0, 9, 1, 0]),
    "no_ids_at_all": dict(lens=[0] * 40),
    "values_all_ones": dict(lens=[3, 4, 5] * 50, valued="ones"),
    "one_value_differs": dict(lens=[3, 4, 5] * 50, valued="one_differs"),
    "real_values": dict(lens=[30] * 700, valued="real"),
    "weights": dict(lens=[2, 9] * 300, valued="real", weighted=True),
    "offset_0_not_0": dict(lens=[4, 0, 6] * 30, first=1234567),
    "many_segments": dict(lens=[39] * 3000),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_record_shapes(dev, ing, ref_crb, tmp_path, name):
    _, _, enc, _ = dev
    off, lab, idx, val, wgt = block(np.random.default_rng(sum(name.encode())), **SHAPES[name])
    rec = enc.encode_host(off, lab, idx, val, wgt)
    check_record(ing, ref_crb, tmp_path, rec, off, lab, idx, val, wgt)
    assert enc.encode_host(off, lab, idx, val, wgt) == rec
    if name in ("values_all_ones", "no_ids_at_all"):
        _, f = fields_of(ing, rec)
        assert f["value"] is None and (name != "no_ids_at_all" or f["index"] is None)


@pytest.mark.gpu
def test_recorded_reference_blocks(dev, ing, ref_crb, tmp_path):
    """the row blocks the reference's Compress was recorded on (tests/golden/ref_ingest.npz)"""
    _, _, enc, _ = dev
    g = np.load(GOLDEN_INGEST)
    count = 0
    while "crb_rec_%d" % count in g:
        i = count
        count += 1
        get = lambda k: g["crb_%d_%s" % (i, k)] if "crb_%d_%s" % (i, k) in g else None   # noqa: E731
        off, lab, idx, val, wgt = get("offset"), get("label"), get("index"), get("value"), get("weight")
        rec = enc.encode_host(off, lab, idx, val, wgt)
        check_record(ing, ref_crb, tmp_path, rec, off, lab, idx, val, wgt)
        # the same fields as the reference's own record, which liblz4 compressed
        _, mine = fields_of(ing, rec)
        _, theirs = fields_of(ing, g["crb_rec_%d" % i].tobytes())
        # (an array of zero elements: absent here, a block of no bytes there; both readers take either)
        assert {k: v or None for k, v in mine.items()} == {k: v or None for k, v in theirs.items()}
    assert count == 9


def host_parse(L, text, train=True):
    cap_rows = text.count(b"\n") + 2
    off = np.zeros(cap_rows + 1, np.uint64)
    lab = np.zeros(cap_rows, np.float32)
    idx = np.zeros(40 * cap_rows, np.uint64)
    buf = C.create_string_buffer(text, len(text)) if text else C.create_string_buffer(1)
    n = L.ingest_parse_criteo(buf, len(text), int(train), 0, cap_rows, 40 * cap_rows, off.ctypes.data, lab.ctypes.data, idx.ctypes.data)
    assert n >= 0, n
    return off[:n + 1].copy(), lab[:n].copy(), idx[:int(off[n])].copy()


TEXT_CASES = ["rows_1", "rows_5000", "rows_65", "only_empty_rows", "criteo_test", "rows_5000", "rows_1"]


@pytest.mark.gpu
def test_text_chunks_in_hbm_give_the_host_arrays_record(dev, ing, ref_crb, tmp_path):
    """one encoder and one chunk object across all cases, growing and shrinking"""
    _, _, enc, tc = dev
    for name in TEXT_CASES:
        text, train = _regular_case(name, np.random.default_rng(sum(name.encode())))
        r = tc.parse_criteo(text, is_train=train)
        assert r is not None, name
        from_hbm = enc.encode_textchunk(tc)
        off, lab, idx = host_parse(ing, text, train)
        assert len(lab) == text.count(b"\n")
        assert from_hbm == enc.encode_host(off, lab, idx), name
        check_record(ing, ref_crb, tmp_path, from_hbm, off, lab, idx)
        assert enc.encode_textchunk(tc) == from_hbm


@pytest.mark.gpu
def test_an_irregular_chunk_is_refused(dev):
    capi, _, enc, tc = dev
    assert tc.parse_criteo(b"1\t2\n") is None
    with pytest.raises(capi.DfhError, match="no regular chunk"):
        enc.encode_textchunk(tc)
