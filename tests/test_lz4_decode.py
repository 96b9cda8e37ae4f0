"""The device LZ4 block decoder (csrc/dfh_lz4dec.hip) through dfh_lz4_decompress: ONE block -> its bytes, or a refusal.

The checker is the product's host decoder (host/lz4_block.h through ingest_lz4_decompress), plus LZ4_decompress_safe of the real
liblz4 where it loads (those comparisons are skipped where it does not; no case depends on it alone).  Everything is exact:
the device's verdict is the host's, the bytes of an accepted block are the host's, and the caller's buffer — filled with a
pattern before the call — is untouched after a refusal.

Blocks are put together here from (literal bytes, offset, match length) items, so that every field of the format sits where the
case wants it: the decoder cuts the compressed bytes into tiles of TILE bytes, reads EVERY position of a tile as if a token
stood there, and walks the true chain from tile to tile, so the edges of a tile and literals that look like tokens are where it
can go wrong.  The matches are not copied in steps of some number of sequences: every output byte gets a pointer to the byte it
copies, and k_lzd_jump halves the pointer chains per launch (round r resolves chains of 2^r), so a chain of dependent matches
is as deep as the case makes it — the dependency case below is 5 000 matches deep, 13 rounds."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096      # LZD_TILE: compressed bytes per workgroup of k_lzd_links / k_lzd_list
FILL = 0xA5      # what the caller's buffer holds before a call


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


def rand(seed, n, below=256):
    return np.random.default_rng(seed).integers(0, below, size=n, dtype=np.uint8).tobytes()


def _length(code_max, length):
    """the bytes behind the token for a length whose nibble holds min(length, 15)"""
    if length < code_max:
        return b""
    rest = length - 15
    return b"\xff" * (rest // 255) + bytes([rest % 255])


def build(items):
    """[(literal bytes, offset, match length)] -> (block, the bytes it stands for).  Match length 0: no match (the last item).
    Offsets and lengths are written as given, valid or not; the model output copies byte by byte where the offset allows"""
    block, out = bytearray(), bytearray()
    for lit, off, ml in items:
        code = ml - 4 if ml else 0
        block.append((min(len(lit), 15) << 4) | min(code, 15))
        block += _length(15, len(lit)) + lit
        out += lit
        if ml:
            block += bytes([off & 255, off >> 8]) + _length(15, code)
            if 1 <= off <= len(out):
                for _ in range(ml):
                    out.append(out[-off])
    return bytes(block), bytes(out)


def seq_bytes(nlit, ml):
    """compressed bytes of a sequence of nlit literals and a match of ml (0: none)"""
    return 1 + len(_length(15, nlit)) + nlit + (2 + len(_length(15, ml - 4)) if ml else 0)


def pad_item(size, seed):
    """a first item (literals, offset 1, match 4) of exactly `size` compressed bytes"""
    for nlit in range(size - 3, max(size - 40, 0), -1):
        if seq_bytes(nlit, 4) == size:
            return (rand(seed, nlit, 250), 1, 4)   # (no 0xFF among them: the runs of the case stand alone)
    raise AssertionError(size)


def host_decode(ing, block, expect):
    out = C.create_string_buffer(bytes([FILL]) * (expect + 1), expect + 1)
    n = ing.ingest_lz4_decompress(block, len(block), out, expect)
    return n, out.raw[:expect]


def accepted(dev, ing, liblz4, block, data):
    """the host accepts `block` as `data`; the device must say and give the same"""
    capi, ctx = dev
    n, out = host_decode(ing, block, len(data))
    assert n == len(data) and out == data, "the case itself is wrong: the host decoder does not give the model's bytes"
    if liblz4 is not None and len(data):
        # (liblz4 also holds a block to the end rules of its own encoder — the last 5 bytes are literals, literals that end within
        # the last 12 bytes end the block — which the host decoder does not ask for: where it refuses, it says nothing)
        out2 = C.create_string_buffer(len(data) + 1)
        r = liblz4.LZ4_decompress_safe(block, out2, len(block), len(data))
        assert r < 0 or (r == len(data) and out2.raw[:len(data)] == data)
    ok, got = capi.lz4_decompress(ctx, block, len(data), FILL)
    assert ok == 1
    if got != data:
        first = next(i for i in range(len(data)) if got[i] != data[i])
        raise AssertionError("the device's bytes differ from the host's from byte %d of %d on" % (first, len(data)))


def refused(dev, ing, block, expect):
    """the host refuses (block, expect); the device must refuse too and leave the buffer alone"""
    capi, ctx = dev
    n, _ = host_decode(ing, block, expect)
    assert n != expect, "the case itself is wrong: the host decoder accepts it"
    ok, got = capi.lz4_decompress(ctx, block, expect, FILL)
    assert ok == 0
    assert got == bytes([FILL]) * expect, "a refused block wrote into the caller's buffer"


# ---------------------------------------------------------------- accepted blocks

@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 14, 15, 16, 15 + 255, 15 + 255 + 1, 9000])
def test_literals_only(dev, ing, liblz4, n):
    """9 000: the run skips two whole tiles, which then have no entry"""
    block, data = build([(rand(n, n), 0, 0)])
    assert data == rand(n, n)
    accepted(dev, ing, liblz4, block, data)


@pytest.mark.gpu
def test_empty_input_follows_the_host_rule(dev, ing):
    capi, ctx = dev
    assert capi.lz4_decompress(ctx, b"", 0, FILL) == (1, b"")
    assert host_decode(ing, b"", 0)[0] == 0
    refused(dev, ing, b"", 3)


@pytest.mark.gpu
@pytest.mark.parametrize("ml", [4, 18, 19, 19 + 255, 70000])
def test_match_lengths(dev, ing, liblz4, ml):
    block, data = build([(rand(ml, 40), 33, ml), (rand(1, 7), 0, 0)])
    assert len(data) == 47 + ml
    accepted(dev, ing, liblz4, block, data)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [1, 2, 3, 4, 7, 8])
def test_matches_that_overlap_their_own_output(dev, ing, liblz4, off):
    for ml in (off + 1, 2 * off + 3, 100, 1000):
        block, data = build([(rand(off, 11), off, max(ml, 4)), (rand(2, 6), 5, 9), (rand(3, 5), 0, 0)])
        accepted(dev, ing, liblz4, block, data)


@pytest.mark.gpu
def test_offset_limits(dev, ing, liblz4):
    # 65 535 exactly, the largest the format writes
    block, data = build([(rand(1, 65535 + 10), 65535, 20), (rand(2, 5), 0, 0)])
    accepted(dev, ing, liblz4, block, data)
    # an offset equal to the output position: the match starts at byte 0
    for nlit in (1, 13, 300):
        block, data = build([(rand(nlit, nlit), nlit, 50), (rand(3, 5), 0, 0)])
        assert data[nlit:nlit + min(nlit, 50)] == data[:min(nlit, 50)]
        accepted(dev, ing, liblz4, block, data)
    block, data = build([(rand(4, 100), 30, 8), (rand(5, 20), 128, 40), (rand(6, 5), 0, 0)])   # 128 = 100 + 8 + 20
    accepted(dev, ing, liblz4, block, data)


EDGE_CASES = {
    # name: (compressed position of the second item's token, the second item)
    "token at 4095": (TILE - 1, (b"abc", 9, 6)),
    "literal length run across the edge": (TILE - 2, (rand(21, 15 + 255 * 2 + 7, 250), 100, 10)),      # run at 4095, 4096, 4097
    "offset bytes at 4095 and 4096": (TILE - 5, (b"xyz", 0x0102, 5)),                                  # token, 3 literals, offset
    "match length run across the edge": (TILE - 4, (b"", 100, 4 + 15 + 255 * 2 + 9)),                  # token, offset, run at 4095 ..
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(EDGE_CASES))
@pytest.mark.parametrize("tile", [1, 2])
def test_fields_on_a_tile_edge(dev, ing, liblz4, name, tile):
    at, item = EDGE_CASES[name]
    at += (tile - 1) * TILE
    items = [pad_item(at, 31), item, (rand(32, 9), 0, 0)]
    block, data = build(items)
    assert seq_bytes(len(items[0][0]), 4) == at and block[at] == (min(len(item[0]), 15) << 4) | min(item[2] - 4, 15)
    if name == "offset bytes at 4095 and 4096":
        assert block[at + 4] == 0x02 and block[at + 5] == 0x01 and (at + 4) % TILE == TILE - 1
    if name == "literal length run across the edge":
        assert block[at + 1:at + 4] == b"\xff\xff\x07" and (at + 2) % TILE == 0
    if name == "match length run across the edge":
        assert block[at + 3:at + 6] == b"\xff\xff\x09" and (at + 4) % TILE == 0
    accepted(dev, ing, liblz4, block, data)


@pytest.mark.gpu
def test_a_chain_of_dependent_matches(dev, ing, liblz4):
    """8 literals, then 5 000 x (4 literals, offset 12, length 8): every match reads what the one before wrote, the pointer
    chains of the last bytes are 5 000 deep (13 jump rounds), the sequences spread over 9 tiles"""
    block, data = build([(rand(0, 8), 8, 4)] + [(rand(k, 4), 12, 8) for k in range(1, 5001)] + [(b"end..", 0, 0)])
    assert len(block) > 8 * TILE
    accepted(dev, ing, liblz4, block, data)
    # the issue's form exactly: the first 8 bytes are literals of the first (4 literals, 12, 8) sequence
    block, data = build([(rand(0, 12), 12, 8)] + [(rand(k, 4), 12, 8) for k in range(1, 5000)] + [(b"tail.", 0, 0)])
    assert len(data) == 8 + 5000 * 12 + 5
    accepted(dev, ing, liblz4, block, data)


@pytest.mark.gpu
@pytest.mark.parametrize("byte", [0xFF, 0xF0, 0x0F, 0x00])
def test_literals_that_look_like_tokens(dev, ing, liblz4, byte):
    """all 0xFF: every position reads as a token with two runs of 255s; all 0xF0: a literal run of 255-sums; the false chains of
    a tile are as many as its positions, the true one is the one that starts at byte 0"""
    lit = bytes([byte])
    block, data = build([(lit * 9000, 4000, 300), (lit * 700, 1, 5000), (lit * 4096, 0, 0)])
    accepted(dev, ing, liblz4, block, data)
    block, data = build([(lit * 20, 7, 40)] * 800 + [(lit * 5, 0, 0)])
    accepted(dev, ing, liblz4, block, data)


def _criteo_like_ids(ing):
    """the ids tests/test_lz4_encode.py compresses in its case d"""
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


@pytest.fixture(scope="module")
def arrays(ing):
    ids = _criteo_like_ids(ing).tobytes()
    assert len(ids) > 500000
    ramp = np.zeros(20001, np.uint64)
    ramp[1:] = np.cumsum(np.random.default_rng(12).integers(20, 40, size=20000))
    return {
        "criteo ids 100000": ids[:100000],
        "criteo ids 1 MiB": (ids * 3)[:1 << 20],
        "zeros 1 MiB": bytes(1 << 20),
        "offsets ramp": ramp.tobytes(),
        "random": rand(99, 300001),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["criteo ids 100000", "criteo ids 1 MiB", "zeros 1 MiB", "offsets ramp", "random"])
def test_blocks_of_the_encoders(dev, ing, liblz4, arrays, name):
    capi, ctx = dev
    data = arrays[name]
    accepted(dev, ing, liblz4, capi.lz4_compress(ctx, data), data)
    if liblz4 is not None:
        from oracle import ingest as oi
        accepted(dev, ing, liblz4, oi.lz4_compress(data), data)


@pytest.mark.gpu
def test_a_small_block_after_a_large_one(dev, ing, liblz4, arrays):
    """a second call on the same context after a larger one.  dfh_lz4_decompress allocates its device arrays per call and frees
    them again, so this checks that calls leave nothing behind that a later one trips over; arrays that GROW and are REUSED belong
    to a chunk object, and that case is tests/test_rec_decode.py's, where one TextChunk decodes a 12 000-row record first and
    every small record after it"""
    capi, ctx = dev
    big = arrays["criteo ids 1 MiB"]
    accepted(dev, ing, liblz4, capi.lz4_compress(ctx, big), big)
    block, data = build([(rand(5, 30), 10, 25), (rand(6, 8), 0, 0)])
    accepted(dev, ing, liblz4, block, data)
    refused(dev, ing, block, len(data) + 1)
    accepted(dev, ing, liblz4, capi.lz4_compress(ctx, big[:70000]), big[:70000])


# ---------------------------------------------------------------- refused blocks

def _good():
    return build([(rand(1, 20), 11, 10), (rand(2, 300), 250, 19 + 255), (rand(3, 6), 0, 0)])


@pytest.mark.gpu
def test_refused_offsets(dev, ing):
    block, data = build([(rand(1, 20), 0, 30), (rand(3, 6), 0, 0)])                  # offset 0
    refused(dev, ing, block, 20 + 30 + 6)
    block, data = build([(rand(1, 20), 21, 30), (rand(3, 6), 0, 0)])                 # one more than the output position
    refused(dev, ing, block, 20 + 30 + 6)
    block, data = build([(rand(1, 20), 11, 30), (rand(2, 5000), 5051, 8), (rand(3, 6), 0, 0)])   # the same, in the second tile
    refused(dev, ing, block, 20 + 30 + 5000 + 8 + 6)
    block, data = build([(rand(1, 20), 11, 30), (rand(2, 5000), 5050, 8), (rand(3, 6), 0, 0)])   # (and the largest that is allowed)
    assert len(data) == 20 + 30 + 5000 + 8 + 6


@pytest.mark.gpu
def test_refused_cuts(dev, ing):
    block, data = _good()
    # inside the last literal run, inside the second one, and inside the first
    for cut in (len(block) - 3, 100, 10):
        refused(dev, ing, block[:cut], len(data))
    # between the two offset bytes of the first match (token, length byte, 20 literals, offset) and of the second
    second = seq_bytes(20, 10)
    assert block[second - 2:second] == bytes([11, 0])
    refused(dev, ing, block[:second - 1], len(data))
    at = second + seq_bytes(300, 19 + 255) - 1 - 1 - 1   # the second offset byte: before the run of the match length (2 bytes)
    assert block[at - 1:at + 1] == bytes([250, 0])
    refused(dev, ing, block[:at], len(data))
    # the whole block is still fine
    assert host_decode(ing, block, len(data))[0] == len(data)


@pytest.mark.gpu
def test_refused_runs_that_reach_the_end(dev, ing):
    refused(dev, ing, b"\xf0" + b"\xff" * 40, 15 + 255 * 40)             # a literal length that never ends
    refused(dev, ing, b"\xf0" + b"\xff" * 9000, 100)                      # ... over three tiles
    refused(dev, ing, b"\x1f" + b"a" + b"\x01\x00" + b"\xff" * 30, 5000)  # a match length that never ends
    refused(dev, ing, b"\xf0", 15)                                        # no byte behind the token at all
    refused(dev, ing, b"\x1f" + b"a" + b"\x01\x00", 20)                   # ... behind the offset


@pytest.mark.gpu
def test_refused_last_sequence_with_a_match(dev, ing):
    block, data = build([(rand(1, 20), 11, 30)])
    refused(dev, ing, block, len(data))
    block, data = build([(rand(1, 20), 11, 19 + 255)])   # (the block ends behind the run of the match length)
    refused(dev, ing, block, len(data))
    block, data = build([(rand(1, 5000), 11, 30)])
    refused(dev, ing, block, len(data))


@pytest.mark.gpu
def test_refused_sizes(dev, ing):
    block, data = _good()
    refused(dev, ing, block, len(data) - 1)
    refused(dev, ing, block, len(data) + 1)
    refused(dev, ing, block, 0)
    block, data = build([(rand(1, 9000), 0, 0)])
    refused(dev, ing, block, 8999)
    refused(dev, ing, block, 9001)


@pytest.mark.gpu
def test_sizes_a_block_cannot_have(dev):
    capi, ctx = dev
    src = C.create_string_buffer(16)
    dst = C.create_string_buffer(16)
    ok = C.c_int(-1)
    assert capi.lib().dfh_lz4_decompress(ctx.h, src, (1 << 31) - (1 << 25), dst, 16, C.byref(ok)) == 1    # DFH_ERR_ARG
    assert capi.lib().dfh_lz4_decompress(ctx.h, src, 16, dst, (1 << 31) - (1 << 25), C.byref(ok)) == 1
