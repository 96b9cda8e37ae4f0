"""text_parse = device of learner = sgd: criteo text parsed on the GPU (csrc/dfh_textparse.hip).

A chunk made of regular rows alone is parsed on the device — offsets, labels and ids equal the host parser's bit for bit — and
every other chunk is reported as not regular and left to the host parser.  Checkers: CriteoChunkParser::ParseSlow through
build/libdifacto_ingest.so (ingest_parse_criteo mode 0), oracle.ingest.parse_criteo, and the reference parser's recorded output
(tests/golden/ref_ingest.npz).  No GPU: the key's values and the combinations Init refuses."""
import ctypes as C
import mmap
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
GOLDEN_INGEST = os.path.join(ROOT, "tests", "golden", "ref_ingest.npz")
TILE = 4096   # bytes per block of the count / position passes (256 lanes x 16 bytes)


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


@pytest.fixture(scope="module")
def ing(built):
    L = C.CDLL(os.path.join(built, "libdifacto_ingest.so"))
    L.ingest_parse_criteo.restype = C.c_long
    L.ingest_parse_criteo.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def dev(built):
    """a context and one text chunk object, reused by every case (its arrays grow and are reused, as in the reader's pool)"""
    from difacto_amd import capi
    ctx = capi.Context(0)
    tc = capi.TextChunk(ctx, 1 << 12)
    yield capi, ctx, tc
    tc.close()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# checkers
# ---------------------------------------------------------------------------------------------------------------------
def host_parse(L, text, train=True):
    """CriteoChunkParser::ParseSlow, the plain loop"""
    cap_rows = text.count(b"\n") + 2
    off = np.zeros(cap_rows + 1, np.uint64)
    lab = np.zeros(cap_rows, np.float32)
    idx = np.zeros(40 * cap_rows, np.uint64)
    buf = C.create_string_buffer(text, len(text)) if text else C.create_string_buffer(1)
    n = L.ingest_parse_criteo(buf, len(text), int(train), 0, cap_rows, 40 * cap_rows, off.ctypes.data, lab.ctypes.data, idx.ctypes.data)
    assert n >= 0, n
    return off[:n + 1].copy(), lab[:n].copy(), idx[:int(off[n])].copy()


def is_regular(text, train=True):
    """the definition of a regular chunk, from the issue's text"""
    ntab = 39 if train else 38
    if not text or not text.endswith(b"\n") or b"\r" in text:
        return False
    for line in text[:-1].split(b"\n"):
        if not line:
            return False
        f = line.split(b"\t")
        if len(f) != ntab + 1:
            return False
        if train:
            if len(f[0]) != 1 or not f[0].isdigit():
                return False
            f = f[1:]
        if any(len(t) > 16 for t in f[:13]):
            return False
        for t in f[13:]:
            if len(t) not in (0, 8) or t[:1] in (b" ", b"\v", b"\f"):
                return False
    return True


def device_parse(dev, text, train=True, address=None):
    """-> None (not regular) or (offset u64, label, ids)"""
    _, _, tc = dev
    r = tc.parse_criteo(text, is_train=train, address=address)
    if r is None:
        return None
    off, lab, nnz = r
    assert int(off[-1]) == nnz
    return off.astype(np.uint64), lab, tc.ids(nnz)


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def check_regular(dev, ing, text, train=True, transcription=True, address=None):
    assert is_regular(text, train)
    got = device_parse(dev, text, train, address)
    assert got is not None, "a regular chunk was handed back"
    want = host_parse(ing, text, train)
    assert len(want[1]) == text.count(b"\n")
    assert same(got, want)
    if transcription:
        from oracle import ingest as oi
        assert same(got, oi.parse_criteo(text, is_train=train))
    return got


# ---------------------------------------------------------------------------------------------------------------------
# text generators
# ---------------------------------------------------------------------------------------------------------------------
def int_token(rng):
    if rng.integers(4) == 0:
        return b""
    tok = str(int(rng.integers(10 ** 12)))[:int(rng.integers(1, 13))].encode()
    return b"-" + tok if rng.integers(9) == 0 else tok


def cat_token(rng):
    return b"%08x" % int(rng.integers(1 << 32)) if rng.integers(6) else b""


def fields(rng, train=True):
    return ([b"%d" % int(rng.integers(0, 10))] if train else []) + [int_token(rng) for _ in range(13)] + [cat_token(rng) for _ in range(26)]


def rows_text(rng, n, train=True):
    return b"".join(b"\t".join(fields(rng, train)) + b"\n" for _ in range(n))


def delimiters(text):
    return [i for i, c in enumerate(text) if c in b"\t\n"]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference parser's recorded texts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_golden_texts(dev, ing):
    g = np.load(GOLDEN_INGEST)
    regular = {0: 1, 1: 0, 2: 0, 3: 1, 4: 1, 5: 0, 6: 0, 7: 0, 8: 1}
    for i in range(9):
        text = g["criteo_text_%d" % i].tobytes()
        train = bool(g["criteo_%d_train" % i])
        assert train == (i != 8)
        assert is_regular(text, train) == bool(regular[i]), i
        got = device_parse(dev, text, train)
        assert (got is not None) == bool(regular[i]), i
        if got is not None:
            want = (g["criteo_%d_offset" % i].astype(np.uint64), g["criteo_%d_label" % i], g["criteo_%d_index" % i])
            assert same(got, want), i


# ---------------------------------------------------------------------------------------------------------------------
# 2. designed regular texts
# ---------------------------------------------------------------------------------------------------------------------
EMPTY_ROW = b"0" + b"\t" * 39 + b"\n"


def _exact_bytes(rng, nbytes):
    """regular rows adding up to exactly nbytes: the last row's integer tokens take what is left"""
    text = b""
    while nbytes - len(text) > len(EMPTY_ROW) + 200:
        row = rows_text(rng, 1)
        text += row if nbytes - len(text) - len(row) >= len(EMPTY_ROW) else EMPTY_ROW
    left = nbytes - len(text) - len(EMPTY_ROW)
    assert 0 <= left <= 13 * 16
    ints = [b"7" * min(16, max(0, left - 16 * i)) for i in range(13)]
    return text + b"\t".join([b"0"] + ints + [b""] * 26) + b"\n"


def _regular_case(name, rng):
    """-> (text, is_train)"""
    if name.startswith("rows_"):
        return rows_text(rng, int(name[5:])), True
    if name.startswith("bytes_"):
        return _exact_bytes(rng, int(name[6:])), True
    if name == "empty_rows":   # all 39 fields empty: alone, several in a row, first and last
        return EMPTY_ROW * 3 + rows_text(rng, 5) + EMPTY_ROW + rows_text(rng, 2) + EMPTY_ROW * 70 + rows_text(rng, 1) + EMPTY_ROW * 2, True
    if name == "only_empty_rows":
        return EMPTY_ROW * 9, True
    if name == "int_lengths":   # every length 0 .. 16 in every integer slot
        out = []
        for r in range(34):
            f = [b"1"] + [bytes(rng.integers(0x30, 0x3a, size=(i + r) % 17, dtype=np.uint8)) for i in range(13)] + [cat_token(rng) for _ in range(26)]
            out.append(b"\t".join(f) + b"\n")
        return b"".join(out), True
    if name == "odd_bytes":   # '-', blanks and bytes 0x80 .. 0xFF in integer tokens; categorical tokens with bytes >= 0x80
        pool = np.array([c for c in range(1, 256) if c not in (9, 10, 13)], np.uint8)
        out = []
        for r in range(60):
            ints = [bytes(rng.choice(pool, size=int(rng.integers(0, 17)))) for _ in range(13)]
            ints[r % 13] = [b"-17", b" 5", b"4 2", b"\x80", b"\xff\xfe", b"- ", b"\xc3\xa9\xc3\xa9"][r % 7]
            cats = []
            for _ in range(26):
                t = bytes(rng.choice(pool[pool >= 0x80], size=8)) if rng.integers(3) else (b"a" + bytes(rng.choice(pool, size=7)))
                cats.append(t if rng.integers(5) else b"")
            out.append(b"\t".join([b"%d" % (r % 10)] + ints + cats) + b"\n")
        return b"".join(out), True
    if name == "longest_row":
        row = b"\t".join([b"9"] + [b"1234567890123456"] * 13 + [b"89abcdef"] * 26) + b"\n"
        return rows_text(rng, 3) + row * 3 + rows_text(rng, 2) + row, True
    if name == "criteo_test":
        return rows_text(rng, 150, train=False), False
    raise KeyError(name)


REGULAR_CASES = ["rows_1", "rows_3", "rows_4", "rows_5", "rows_63", "rows_64", "rows_65", "rows_5000",
                 "bytes_%d" % (TILE - 1), "bytes_%d" % TILE, "bytes_%d" % (TILE + 1),
                 "empty_rows", "only_empty_rows", "int_lengths", "odd_bytes", "longest_row", "criteo_test"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", REGULAR_CASES)
def test_designed_regular_texts(dev, ing, name):
    """rows_3 / 4 / 5: one block of the field passes holds 4 rows; bytes_*: one tile of the count / position passes; rows_5000:
    ~290 tiles and 1 250 row blocks, several blocks of the library scans"""
    text, train = _regular_case(name, np.random.default_rng(sum(name.encode())))
    if name.startswith("bytes_"):
        assert len(text) == int(name[6:])
    off, lab, idx = check_regular(dev, ing, text, train)
    if name == "only_empty_rows":
        assert len(idx) == 0 and not off.any()
    if name == "empty_rows":
        assert (np.diff(off.astype(np.int64)) == 0).sum() == 76


@pytest.mark.gpu
def test_delimiters_on_load_and_tile_edges(dev, ing):
    """the same rows behind a first integer token of 0 .. 16 bytes: every delimiter visits every position of a lane's 16-byte
    load, and the delimiters next to the first tile boundary fall on its last byte and on the first byte of the next tile"""
    rng = np.random.default_rng(5)
    tail = rows_text(rng, 40)
    f = fields(rng)
    seen = set()
    for shift in range(17):
        f[1] = b"3" * shift
        text = b"\t".join(f) + b"\n" + tail
        d = delimiters(text)
        seen |= {"last_of_lane"} if any(p % 16 == 15 for p in d) else set()
        seen |= {"first_of_lane"} if any(p % 16 == 0 for p in d) else set()
        seen |= {"tile_last"} if TILE - 1 in d else set()
        seen |= {"tile_first"} if TILE in d else set()
        nl = [p for p in d if text[p] == 10]
        seen |= {"row_spans_tiles"} if any(a < TILE <= b for a, b in zip(nl, nl[1:]) if b - a > 1) else set()
        check_regular(dev, ing, text, transcription=False)
    assert seen == {"last_of_lane", "first_of_lane", "tile_last", "tile_first", "row_spans_tiles"}, seen


@pytest.mark.gpu
def test_text_at_the_end_of_its_allocation(dev, ing):
    """the upload reads len bytes and not one more: the text's last byte is the last byte of a mapping"""
    text = rows_text(np.random.default_rng(9), 33)
    size = (len(text) + mmap.PAGESIZE - 1) // mmap.PAGESIZE * mmap.PAGESIZE
    m = mmap.mmap(-1, size)
    m[size - len(text):] = text
    hold = C.c_char.from_buffer(m)
    try:
        check_regular(dev, ing, text, transcription=False, address=C.addressof(hold) + size - len(text))
    finally:
        del hold
        m.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. designed irregular texts
# ---------------------------------------------------------------------------------------------------------------------
def _set_field(row, j, tok):
    f = row[:-1].split(b"\t")
    f[j] = tok
    return b"\t".join(f) + b"\n"


DEFECTS = {
    "cr": lambda r: r[:-1] + b"\r\n",
    "empty_line": lambda r: b"\n" + r,
    "tab_too_few": lambda r: r[:r.rindex(b"\t")] + r[r.rindex(b"\t") + 1:],
    "tab_too_many": lambda r: r[:-1] + b"\t\n",
    "label_10": lambda r: _set_field(r, 0, b"10"),
    "label_minus_1": lambda r: _set_field(r, 0, b"-1"),
    "label_half": lambda r: _set_field(r, 0, b"0.5"),
    "label_empty": lambda r: _set_field(r, 0, b""),
    "label_letter": lambda r: _set_field(r, 0, b"x"),
    "int_17_bytes": lambda r: _set_field(r, 4, b"12345678901234567"),
    "cat_7_bytes": lambda r: _set_field(r, 20, b"0123456"),
    "cat_9_bytes": lambda r: _set_field(r, 39, b"012345678"),
    "cat_starts_with_blank": lambda r: _set_field(r, 14, b" 1234567"),
    "cat_starts_with_vt": lambda r: _set_field(r, 30, b"\v1234567"),
    "cat_starts_with_ff": lambda r: _set_field(r, 39, b"\f1234567"),
}


@pytest.fixture(scope="module")
def base_rows():
    rng = np.random.default_rng(77)
    return [b"\t".join(fields(rng)) + b"\n" for _ in range(300)]


@pytest.mark.gpu
@pytest.mark.parametrize("defect", sorted(DEFECTS) + ["no_final_newline", "empty_line_at_the_end", "too_many_then_too_few", "empty_text"])
def test_designed_irregular_texts(dev, ing, base_rows, defect):
    """one defect in the first, a middle or the last of ~300 regular rows: the chunk is handed back"""
    assert device_parse(dev, b"".join(base_rows)) is not None
    for k in (0, 150, 299):
        rows = list(base_rows)
        if defect == "empty_text":
            text = b""
        elif defect == "no_final_newline":
            text = b"".join(rows[:k + 1])[:-1]
        elif defect == "empty_line_at_the_end":
            text = b"".join(rows[:k + 1]) + b"\n"
        elif defect == "too_many_then_too_few":   # the totals are those of a regular chunk
            k = min(k, 298)
            rows[k] = DEFECTS["tab_too_many"](rows[k])
            rows[k + 1] = DEFECTS["tab_too_few"](rows[k + 1])
            text = b"".join(rows)
            assert text.count(b"\t") == 39 * 300 and text.count(b"\n") == 300
        else:
            rows[k] = DEFECTS[defect](rows[k])
            text = b"".join(rows)
        assert not is_regular(text)
        assert device_parse(dev, text) is None, (defect, k)
    # the object is as good as new afterwards
    assert device_parse(dev, b"".join(base_rows)) is not None


# ---------------------------------------------------------------------------------------------------------------------
# 4. fuzz
# ---------------------------------------------------------------------------------------------------------------------
def _fuzz_text(rng):
    train = bool(rng.integers(5))
    n = int(rng.integers(1, 400 if rng.integers(8) == 0 else 40))
    rows = []
    for _ in range(n):
        f = fields(rng, train)
        o = 1 if train else 0
        if rng.integers(6) == 0:   # still regular: junk in integer fields, long integer tokens, odd categorical bytes
            f[o + int(rng.integers(13))] = [b"1 2", b"-", b"1234567890123456", b"\xe9", b"+7.5e3"][int(rng.integers(5))]
            f[o + 13 + int(rng.integers(26))] = [b"zzzzzzzz", b"a b c d ", b"\xff" * 8][int(rng.integers(3))]
        rows.append(b"\t".join(f) + b"\n")
    if rng.integers(100) < 38:   # one or two defects somewhere
        for _ in range(int(rng.integers(1, 3))):
            k = int(rng.integers(n))
            kind = int(rng.integers(10))
            r = rows[k]
            if kind == 0:
                r = r[:-1] + b"\r\n"
            elif kind == 1:
                r = b"\n" + r
            elif kind == 2:
                r = r.replace(b"\t", b"", 1)
            elif kind == 3:
                r = r[:-1] + b"\t\n"
            elif kind == 4 and train:
                r = _set_field(r, 0, [b"12", b"-1", b"0.5", b"", b"1e0"][int(rng.integers(5))])
            elif kind == 5:
                r = _set_field(r, (1 if train else 0) + int(rng.integers(13)), b"9" * int(rng.integers(17, 40)))
            elif kind == 6:
                r = _set_field(r, (1 if train else 0) + 13 + int(rng.integers(26)), b"abcdef0123"[:int(rng.choice([1, 5, 7, 9, 10]))])
            elif kind == 7:
                r = _set_field(r, (1 if train else 0) + 13 + int(rng.integers(26)), [b" ", b"\v", b"\f"][int(rng.integers(3))] + b"1234567")
            elif kind == 8:
                r = r[:-1]   # two rows on one line; the last row: no final newline
            elif kind == 9:
                r = r[:int(rng.integers(1, len(r)))] + b"\n"   # a short row
            rows[k] = r
    return b"".join(rows), train


@pytest.mark.gpu
def test_fuzz_flag_equals_the_definition(dev, ing):
    rng = np.random.default_rng(2024)
    nreg = nirr = 0
    total = 160
    for it in range(total):
        text, train = _fuzz_text(rng)
        got = device_parse(dev, text, train)
        reg = is_regular(text, train)
        assert (got is not None) == reg, (it, text[:200])
        if reg:
            nreg += 1
            assert same(got, host_parse(ing, text, train)), it
        else:
            nirr += 1
    assert nreg * 2 >= total and nirr * 4 >= total, (nreg, nirr)


# ---------------------------------------------------------------------------------------------------------------------
# 5. device and host slices in one row buffer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("valued", [False, True])
def test_mixed_slices_fill_the_same_buffer(dev, ing, valued):
    """dfh_rowbuf_load_slices with slices of parsed chunks (device to device, ranges that start mid-chunk) between host slices,
    against dfh_rowbuf_load_host of the assembled arrays: every minibatch gathered out of the two buffers is the same"""
    capi, ctx, _ = dev
    rng = np.random.default_rng(31)
    texts = [rows_text(rng, n) for n in (200, 150, 120)]
    host = [host_parse(ing, t) for t in texts]
    chunks = [capi.TextChunk(ctx, 1 << 10) for _ in range(2)]
    for tc, t, h in zip(chunks, texts, host):
        r = tc.parse_criteo(t)
        assert r is not None and np.array_equal(r[0], h[0].astype(np.uint32))
    # a fourth source with values of its own (valued), never parsed from text
    n4 = 90
    off4 = np.zeros(n4 + 1, np.uint64)
    off4[1:] = np.cumsum(rng.integers(0, 20, size=n4))
    idx4 = rng.integers(0, 2 ** 40, size=int(off4[-1]), dtype=np.uint64)
    val4 = rng.normal(size=int(off4[-1])).astype(np.float32) if valued else None
    lab4 = (rng.random(n4) < 0.3).astype(np.float32)
    # (source, first row, rows): device A mid-chunk, host C mid-chunk, device B from its start, host D, device A's head
    plan = [(0, 50, 150), (2, 10, 90), (1, 0, 120), (3, 0, n4), (0, 0, 50), (1, 149, 1)]
    lens, labs, idxs, vals, slices = [], [], [], [], []
    for src, r0, n in plan:
        o, lb, ix = (off4, lab4, idx4) if src == 3 else host[src]
        lo, hi = int(o[r0]), int(o[r0 + n])
        lens.append(np.diff(o[r0:r0 + n + 1].astype(np.int64)))
        labs.append(lb[r0:r0 + n])
        idxs.append(ix[lo:hi])
        vals.append(val4[lo:hi] if (src == 3 and valued) else np.ones(hi - lo, np.float32))
        if src in (0, 1):
            slices.append((chunks[src], lo, hi - lo))
        else:
            slices.append((ix[lo:hi], val4[lo:hi] if (src == 3 and valued) else None))
    nrows = sum(n for _, _, n in plan)
    offset = np.zeros(nrows + 1, np.uint64)
    offset[1:] = np.cumsum(np.concatenate(lens))
    label, index = np.concatenate(labs), np.concatenate(idxs)
    value = np.concatenate(vals) if valued else None
    nnz = int(offset[-1])
    assert len(index) == nnz
    rb_ref, rb_mix = capi.RowBuf(ctx, nrows, nnz), capi.RowBuf(ctx, nrows, nnz)
    rb_ref.load_host(offset, index, value)
    rb_mix.load_slices(offset, slices)
    for rb in (rb_ref, rb_mix):
        rb.set_labels(label)
    ctx.set_pipeline(1)
    picks = [rng.permutation(nrows)[:257], np.arange(nrows), np.array([149, 150, 239, 240, 359, 360, 449, 450, nrows - 1]),
             rng.permutation(nrows)[:64]]
    out = []
    for rb in (rb_ref, rb_mix):
        tb = capi.Table(ctx, 1 << 16, V_dim=4, init_mode=capi.INIT_HASH, V_threshold=0, lr=0.2, l1=0.01)
        bt = capi.Batch(ctx, nrows, max(nnz, 1))
        res = []
        for how in ("gather_rows", "prepare_rows", "prepare_cached"):
            for rows in picks:
                rows = rows.astype(np.uint32)
                ln = np.diff(offset.astype(np.int64))[rows]
                off = np.zeros(len(rows) + 1, np.uint64)
                off[1:] = np.cumsum(ln)
                if how == "gather_rows":
                    bt.gather_rows(off, label[rows], [(rb, rows)])
                    bt.localize()
                elif how == "prepare_rows":
                    bt.prepare_rows(tb, off, label[rows], [(rb, rows)])
                else:
                    bt.prepare_cached(tb, [(rb, rows)])
                d_off, d_lab = bt.get_rows()
                assert np.array_equal(d_off, off.astype(np.uint32)) and d_lab.tobytes() == label[rows].tobytes()
                loc = bt.get_localized()
                bt.sgd_step(tb, is_train=True, push_cnt=True)
                res.append((d_off, d_lab, loc["feaids"], loc["index"], loc["feacnt"], bt.pred()))
        # the gathered ids themselves: the sorted unique keys and the per-nonzero ranks give them back
        want = np.sort(np.unique(np.array([capi.reverse_bytes(int(x)) for x in index[:64]], np.uint64)))
        assert np.isin(want, np.concatenate([r[2] for r in res])).all()
        out.append(res)
        bt.close()
        tb.close()
    for a, b in zip(*out):
        assert same(a, b)
    for o in (rb_ref, rb_mix, *chunks):
        o.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the command line
# ---------------------------------------------------------------------------------------------------------------------
def _difacto(built, *args, env=None, data=DATA, timeout=300):
    return subprocess.run([os.path.join(built, "difacto"), "data_in=" + data] + list(args), capture_output=True, text=True, timeout=timeout,
                          cwd=ROOT, env=env)


@pytest.fixture(scope="module")
def criteo_files(tmp_path_factory):
    """3 000 generated rows; the same with one CRLF row in the middle"""
    d = tmp_path_factory.mktemp("criteo_cli")
    rng = np.random.default_rng(7)
    rows = []
    for _ in range(3000):
        ints = [b"" if rng.random() < 0.2 else b"%d" % int(rng.integers(0, 50)) for _ in range(13)]
        cats = [b"" if rng.random() < 0.15 else b"%08x" % int(rng.integers(0, 40)) for _ in range(26)]
        rows.append(b"\t".join([b"%d" % int(rng.random() < 0.3)] + ints + cats) + b"\n")
    clean, crlf = d / "clean.txt", d / "crlf.txt"
    clean.write_bytes(b"".join(rows))
    rows[1500] = rows[1500][:-1] + b"\r\n"
    crlf.write_bytes(b"".join(rows))
    return {"clean": str(clean), "crlf": str(crlf)}


def _model_records(blob):
    """model_out as (header, records sorted by key), every byte of it.  The file lists the table's rows in the order the
    keys were first inserted, which the insert's atomics decide anew in every run (two runs with text_parse=host differ in
    it too; tests/test_sgd_data_cache.py sorts by key for the same reason): the comparison is of the records' bytes, in key
    order.  Layout (dfh_table_save, with optimiser state): "DFHM", version, V_dim, aux = 1, count; per entry key u64, w,
    {fea_cnt, sqrt_g, z}, has_V i32, then V and its accumulators (2 x V_dim floats) iff has_V"""
    head, k, aux, n = blob[:24], int.from_bytes(blob[8:12], "little"), int.from_bytes(blob[12:16], "little"), int.from_bytes(blob[16:24], "little")
    assert blob[:4] == b"DFHM" and aux == 1 and k == 4
    recs, at = [], 24
    for _ in range(n):
        has_v = int.from_bytes(blob[at + 24:at + 28], "little")
        size = 28 + (8 * k if has_v else 0)
        recs.append(blob[at:at + size])
        at += size
    assert at == len(blob) and n > 100
    recs.sort(key=lambda r: int.from_bytes(r[:8], "little"))
    return head, recs


CLI_CONFIGS = {"plain": [], "neg_sampling": ["neg_sampling=0.7"], "data_cache": ["data_cache=hbm"]}


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["clean", "crlf"])
@pytest.mark.parametrize("config", sorted(CLI_CONFIGS))
def test_cli_results_do_not_depend_on_where_the_text_is_parsed(built, tmp_path, criteo_files, config, which):
    """Training lines string for string and model_out byte for byte (its records in key order); chunks of 4 096 bytes: many per shuffle buffer, slices
    that cross buffers; the chunk with the CRLF row falls back to the host parser and the log says so"""
    env = dict(os.environ, DIFACTO_CHUNK_BYTES="4096")
    runs = {}
    for mode in ("host", "device"):
        model = tmp_path / ("model_" + mode)
        r = _difacto(built, "data_format=criteo", "batch_size=300", "shuffle=2", "V_dim=4", "max_num_epochs=2", "V_threshold=2", "l1=.1",
                     "lr=.1", "stop_rel_objv=0", "stop_val_auc=-1e30", "model_out=%s" % model, "text_parse=" + mode, *CLI_CONFIGS[config],
                     env=env, data=criteo_files[which])
        assert r.returncode == 0, r.stderr[-3000:]
        runs[mode] = (re.findall(r" - (Training: .*)$", r.stderr, re.M), model.read_bytes(), r.stderr)
    (lines_h, model_h, log_h), (lines_d, model_d, log_d) = runs["host"], runs["device"]
    assert len(lines_h) == 2 and lines_h == lines_d, "\n".join(lines_h + ["--"] + lines_d)
    assert len(model_h) > 1000 and len(model_h) == len(model_d) and _model_records(model_h) == _model_records(model_d)
    assert "text_parse" not in log_h
    counts = re.findall(r"text_parse=device: (\d+) of (\d+) chunks of \S+ parsed on the device, (\d+) fell back to the host parser", log_d)
    assert counts, log_d[-3000:]
    on_device, chunks, fell_back = (sum(int(c[i]) for c in counts) for i in range(3))
    assert on_device > 100 and on_device + fell_back == chunks
    parsed_epochs = 1 if config == "data_cache" else 2
    if which == "crlf":
        assert fell_back == parsed_epochs and "WARNING" in log_d and "were parsed on the host" in log_d, log_d[-3000:]
    else:
        assert fell_back == 0 and "were parsed on the host" not in log_d


# ---------------------------------------------------------------------------------------------------------------------
# 7. the key's values and the combinations Init refuses (no GPU: refused before the device is touched)
# ---------------------------------------------------------------------------------------------------------------------
REQUIRED = ["batch_size=25", "V_dim=4"]


def test_unknown_value_is_fatal(built):
    r = _difacto(built, *REQUIRED, "text_parse=disk")
    assert r.returncode != 0 and "text_parse=disk" in r.stderr and "host" in r.stderr and "device" in r.stderr, r.stderr[-2000:]


def test_libsvm_is_refused(built):
    r = _difacto(built, *REQUIRED, "text_parse=device", "data_format=libsvm", "shuffle=2")
    assert r.returncode != 0 and "text_parse=device with data_format=libsvm" in r.stderr and "criteo" in r.stderr, r.stderr[-2000:]


def test_literal_path_is_refused(built):
    r = _difacto(built, *REQUIRED, "text_parse=device", "data_format=criteo", "shuffle=2", "device_path=literal")
    assert r.returncode != 0 and "text_parse=device with device_path=literal" in r.stderr, r.stderr[-2000:]


def test_a_rank_is_refused(built, tmp_path):
    env = dict(os.environ, DMLC_ROLE="worker", DMLC_NUM_WORKER="2", DIFACTO_RANK="0", DIFACTO_DEVICE="0", DIFACTO_COMM="file",
               DIFACTO_RENDEZVOUS=str(tmp_path))
    r = _difacto(built, *REQUIRED, "text_parse=device", "data_format=criteo", "shuffle=2", env=env)
    assert r.returncode != 0 and "text_parse=device with a sharded store" in r.stderr, r.stderr[-2000:]


def test_lbfgs_is_refused(built):
    r = _difacto(built, *REQUIRED, "text_parse=device", "data_format=criteo", "learner=lbfgs")
    assert r.returncode != 0 and "text_parse=device with learner=lbfgs" in r.stderr and "learner=sgd" in r.stderr, r.stderr[-2000:]


def test_no_shuffle_buffer_is_refused(built):
    r = _difacto(built, *REQUIRED, "text_parse=device", "data_format=criteo", "shuffle=0")
    assert r.returncode != 0 and "text_parse=device without a shuffle buffer" in r.stderr, r.stderr[-2000:]
