"""The device LZ4 block encoder (csrc/dfh_lz4enc.hip) through dfh_lz4_compress: one array -> ONE block.

Every case is checked four ways: (a) the product's decoder (host/lz4_block.h through ingest_lz4_decompress) returns the input,
(b) so does LZ4_decompress_safe of the real liblz4 where it loads, (c) the size is within LZ4_compressBound, (d) a second call
gives the same bytes.  On top of that the block is walked sequence by sequence here (the format description at the top of
host/lz4_block.h) and the end-of-block rules LZ4_decompress_safe relies on are asserted: the last sequence is literals only, the
last 5 bytes are literals, no match starts within the last 12 bytes, offsets are 1 .. 65535 and never reach before the block."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 4096   # bytes per segment of the encoder (LZ_SEG): a wave per segment, matches do not run over a segment's end

# criteo-like ids (case d): the encoder's size relative to liblz4's LZ4_compress_default of the same bytes, measured on an
# MI355X (profiles/convert_ratio.txt); the test allows a tenth more, so that a later regression of the match finder shows
MEASURED_RATIO_TO_LIBLZ4 = 0.9999


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
    L.ingest_parse_criteo.restype = C.c_long
    L.ingest_parse_criteo.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def dev(built):
    from difacto_amd import capi
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


@pytest.fixture(scope="module")
def liblz4():
    from oracle import ingest as oi
    try:
        return oi.liblz4()
    except OSError:
        return None


def sequences(block, n):
    """-> [(literal length, match length, offset)], the last one (lit, 0, 0); asserts the format and the end rules"""
    seqs, ip, op = [], 0, 0
    while True:
        assert ip < len(block), "the block ends where a token should be"
        token = block[ip]
        ip += 1
        lit = token >> 4
        if lit == 15:
            while True:
                b = block[ip]
                ip += 1
                lit += b
                if b != 255:
                    break
        ip += lit
        op += lit
        assert ip <= len(block) and op <= n
        if ip == len(block):
            assert token & 15 == 0, "the last sequence carries a match length"
            seqs.append((lit, 0, 0))
            break
        offset = block[ip] | (block[ip + 1] << 8)
        ip += 2
        mlen = token & 15
        if mlen == 15:
            while True:
                b = block[ip]
                ip += 1
                mlen += b
                if b != 255:
                    break
        mlen += 4
        assert 1 <= offset <= 65535 and offset <= op, (offset, op)
        assert op + 12 <= n, "a match starts within the last 12 bytes"
        op += mlen
        assert op + 5 <= n, "a match covers one of the last 5 bytes"
        seqs.append((lit, mlen, offset))
    assert op == n
    assert n < 13 and len(seqs) == 1 or n >= 13 and seqs[-1][0] >= 5
    return seqs


def check(dev, ing, liblz4, data):
    """-> (block, sequences) after checks (a) .. (d) and the end rules"""
    capi, ctx = dev
    data = bytes(data)
    n = len(data)
    block = capi.lz4_compress(ctx, data)
    assert len(block) <= n + n // 255 + 16                                  # (c)
    out = C.create_string_buffer(n + 1)
    assert ing.ingest_lz4_decompress(block, len(block), out, n) == n and out.raw[:n] == data          # (a)
    if liblz4 is not None:                                                  # (b)
        out2 = C.create_string_buffer(n + 1)
        assert liblz4.LZ4_decompress_safe(block, out2, len(block), n) == n and out2.raw[:n] == data
    assert capi.lz4_compress(ctx, data) == block                            # (d)
    return block, sequences(block, n)


def rand(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


SIZES = [1, 4, 5, 11, 12, 13, 16, 20, SEG - 1, SEG, SEG + 1, 2 * SEG + 5, 65535, 65536, 65541, (1 << 20) + 3]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes_random_and_equal_bytes(dev, ing, liblz4, n):
    _, seqs = check(dev, ing, liblz4, rand(n, n))
    block, seqs = check(dev, ing, liblz4, b"\x5a" * n)
    if n < 13:
        assert seqs == [(n, 0, 0)]
    if n >= 16:   # a run is found: 4 literals, matches at distance 4 up to the last 5 bytes
        assert seqs[0][0] == 4 and all(s[2] == 4 for s in seqs[:-1]) and seqs[-1][0] == 5
        assert sum(s[1] for s in seqs) == n - 9
        assert len(block) <= 32 + n // 128


@pytest.mark.gpu
@pytest.mark.parametrize("n", [13, 14, 15, 16, 17, 18, 19, 20])
def test_equal_bytes_at_the_end_rules(dev, ing, liblz4, n):
    """13 .. 15 bytes: the only word a match could start at is the first; from 16 on a match of n - 9 bytes fits"""
    _, seqs = check(dev, ing, liblz4, b"\x00" * n)
    assert seqs == ([(n, 0, 0)] if n < 16 else [(4, n - 9, 4), (5, 0, 0)])


@pytest.mark.gpu
@pytest.mark.parametrize("code", [14, 15, 15 + 254, 15 + 255, 15 + 256, 15 + 510])
def test_match_length_codes(dev, ing, liblz4, code):
    """equal bytes: 4 literals, ONE match of n - 9 bytes, 5 literals; n chosen so that length - 4 is the code under test"""
    n = code + 4 + 9
    _, seqs = check(dev, ing, liblz4, b"\xa7" * n)
    assert seqs == [(4, code + 4, 4), (5, 0, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("lit", [14, 15, 16, 269, 270, 271])
def test_literal_length_codes(dev, ing, liblz4, lit):
    """`lit` incompressible bytes, then 16 bytes that repeat what lies `dist` before them (8 for the short runs — one element
    back, the repeat overlaps itself; 264 for the long ones), then 12 more literals: the first sequence has exactly `lit` literals"""
    dist = 8 if lit < 100 else 264
    rng = np.random.default_rng(lit)
    data = bytearray(rng.integers(0, 256, size=lit, dtype=np.uint8).tobytes())
    data[lit - 1] = data[lit - 1 - dist] ^ 0xFF          # the repeat starts at `lit`, not before
    for _ in range(16):
        data.append(data[len(data) - dist])
    tail = bytearray(rng.integers(0, 256, size=12, dtype=np.uint8).tobytes())
    tail[0] = data[len(data) - dist] ^ 0xFF               # ... and ends after 16 bytes
    data += tail
    _, seqs = check(dev, ing, liblz4, data)
    assert seqs == [(lit, 16, dist), (12, 0, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("dist", [65535, 65536])
def test_offset_limit(dev, ing, liblz4, dist):
    """64 random bytes, incompressible filler, the same 64 bytes `dist` behind their first copy: both round-trip, and nothing
    refers 65 536 back (the walk above asserts offsets <= 65535; here: no match reaches the first copy at all at 65 536)"""
    a = rand(1, 64)
    data = a + rand(2, dist - 64) + a + rand(3, 40)
    _, seqs = check(dev, ing, liblz4, data)
    if dist == 65536:
        op = 0
        for lit, mlen, off in seqs:
            op += lit
            assert mlen == 0 or op - off >= 64, "a match refers into the first copy of A, 65 536 bytes back"
            op += mlen


@pytest.mark.gpu
def test_tail(dev, ing, liblz4):
    """the last 16 bytes repeat the 16 before them (the match stops 5 bytes short of the end); a repeat that would end 4, 5
    and 6 bytes before the end (ends there only where the rules allow)"""
    base = rand(4, 200)
    _, seqs = check(dev, ing, liblz4, base + base[-16:])
    assert seqs[-2][1] == 11 and seqs[-2][2] == 16 and seqs[-1][0] == 5
    for left in (4, 5, 6):
        rep = base[-32:]
        tail = bytearray(rand(5 + left, left))
        tail[0] = base[200 - 32] ^ 0xFF   # (what would continue the repeat)
        _, seqs = check(dev, ing, liblz4, base + rep + bytes(tail))
        assert seqs[-2][2] == 32 and seqs[-2][1] == min(32, 32 + left - 5) and seqs[-1][0] == max(left, 5)


@pytest.mark.gpu
def test_segment_seams(dev, ing, liblz4):
    # a run of equal elements that starts in one segment and ends in the third
    data = rand(6, SEG - 400) + b"\x11\x22\x33\x44" * ((SEG + 800) // 4) + rand(7, SEG)
    _, seqs = check(dev, ing, liblz4, data)
    assert sum(s[1] for s in seqs) >= SEG + 800 - 4 - 3
    # a segment of literals only between two segments with matches: its bytes are literals of the third segment's first sequence
    data = b"\x01\x00\x00\x00" * (SEG // 4) + rand(8, SEG) + b"\x02\x00\x00\x00" * (SEG // 4)
    _, seqs = check(dev, ing, liblz4, data)
    assert any(s[0] >= SEG for s in seqs[:-1])
    # the last segment shorter than 13 bytes
    for extra in (1, 7, 12):
        _, seqs = check(dev, ing, liblz4, b"\x09" * SEG + rand(9, extra))
        assert seqs[-1][0] >= max(extra, 5)
    # nothing but literals over many segments, then one match in the last
    _, seqs = check(dev, ing, liblz4, rand(10, 5 * SEG + 100) + b"\x00" * 64)
    assert seqs[0][0] >= 5 * SEG + 100


def _criteo_like_ids(ing):
    """the ids of the criteo text tests/test_text_parse.py's command-line tests generate (few distinct tokens per field)"""
    rng = np.random.default_rng(7)
    rows = []
    for _ in range(3000):
        ints = [b"" if rng.random() < 0.2 else b"%d" % int(rng.integers(0, 50)) for _ in range(13)]
        cats = [b"" if rng.random() < 0.15 else b"%08x" % int(rng.integers(0, 40)) for _ in range(26)]
        rows.append(b"\t".join([b"%d" % int(rng.random() < 0.3)] + ints + cats) + b"\n")
    text = b"".join(rows)
    off = np.zeros(3002, np.uint64)
    lab = np.zeros(3001, np.float32)
    idx = np.zeros(40 * 3001, np.uint64)
    n = ing.ingest_parse_criteo(text, len(text), 1, 0, 3001, 40 * 3001, off.ctypes.data, lab.ctypes.data, idx.ctypes.data)
    assert n == 3000
    return idx[:int(off[n])].copy()


@pytest.mark.gpu
def test_array_shaped_inputs(dev, ing, liblz4, capsys):
    """the arrays of a row block, with conditions that follow from the format (liblz4 itself meets them)"""
    rng = np.random.default_rng(12)
    # a) constant labels: one match per segment
    raw = np.ones(5000, np.float32).tobytes()
    block, _ = check(dev, ing, liblz4, raw)
    assert len(block) <= len(raw) // 16
    # b) offsets: an element shares its 6 high bytes with its predecessor: token + 2 literals + offset = 5 bytes per 8
    off = np.zeros(5001, np.uint64)
    off[1:] = np.cumsum(rng.integers(20, 40, size=5000))
    raw = off.tobytes()
    block, _ = check(dev, ing, liblz4, raw)
    assert len(block) <= 0.75 * len(raw)
    # c) random ids: nothing to find; check() holds the block to the bound
    block, seqs = check(dev, ing, liblz4, rng.integers(0, 2 ** 64 - 1, size=100000, dtype=np.uint64).tobytes())
    # d) criteo-like ids, against liblz4 on the same bytes
    from oracle import ingest as oi
    raw = _criteo_like_ids(ing).tobytes()
    block, _ = check(dev, ing, liblz4, raw)
    if liblz4 is None:
        return
    theirs = len(oi.lz4_compress(raw))
    with capsys.disabled():
        print("\ncriteo-like ids: %d bytes raw, device encoder %d (%.4f of raw), liblz4 %d (%.4f of raw), ratio %.4f"
              % (len(raw), len(block), len(block) / len(raw), theirs, theirs / len(raw), len(block) / theirs))
    assert len(block) <= 1.1 * MEASURED_RATIO_TO_LIBLZ4 * theirs


@pytest.mark.gpu
def test_a_small_destination_is_refused(dev):
    capi, ctx = dev
    data = rand(13, 1000)
    src = C.create_string_buffer(data, len(data))
    dst = C.create_string_buffer(100)
    out = C.c_size_t(0)
    assert capi.lib().dfh_lz4_compress(ctx.h, src, len(data), dst, 100, C.byref(out)) != 0
    assert b"dst holds 100" in capi.lib().dfh_last_error()
