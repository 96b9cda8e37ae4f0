"""A model table as sorted text on the device (csrc/dfh_dumptext.hip, csrc/dfh_dumptext_fmt.h) through capi.Table.import_ and
capi.ModelDump: one line "<id>\\t<w>[\\t<V_j>]\\n" per entry with w != 0 or V, ascending in the printed id, against the C library
itself (snprintf through ctypes: "%llu", "\\t%.9g").  Text must be EQUAL, byte for byte.

An entry takes P = min(64, pow2 >= 1 + V_dim) lanes, a lane per value and round, so V_dim sits on one round of a wave, exactly
64 values, 65, and across 128; a tile of the two format kernels is ModelDump.tile entries (by V_dim), a tile's text starts at
whatever byte the tile before it ends, and the entry counts sit on the tile's edges."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_libc = ctypes.CDLL(None)
ERR_ARG, ERR_STATE = 1, 4   # DFH_ERR_ARG, DFH_ERR_STATE of include/difacto_hip.h
U64 = np.uint64


def field(v):
    """the oracle: what fprintf("\\t%.9g", v) writes for the float v"""
    buf = ctypes.create_string_buffer(40)
    n = _libc.snprintf(buf, 40, b"\t%.9g", ctypes.c_double(float(v)))
    assert 0 < n < 40
    return buf.raw[:n]


def id_text(i):
    buf = ctypes.create_string_buffer(40)
    n = _libc.snprintf(buf, 40, b"%llu", ctypes.c_ulonglong(int(i)))
    return buf.raw[:n]


def rev(x):
    """ReverseBytes (include/difacto/base.h): the nibbles of a 64-bit word in reverse order"""
    x = np.asarray(x, U64).byteswap()
    return ((x & U64(0x0F0F0F0F0F0F0F0F)) << U64(4)) | ((x & U64(0xF0F0F0F0F0F0F0F0)) >> U64(4))


def render(ids, w, has, V):
    """the expected text of entries that are all kept, in the order given"""
    out = []
    for i in range(len(ids)):
        out.append(id_text(ids[i]) + field(w[i]) + (b"".join(field(x) for x in V[i]) if has[i] and V is not None else b"") + b"\n")
    return out


# ids of every digit count 1 .. 20, as they stand in a data file
SPECIAL = [1, 9] + [x for d in range(1, 20) for x in (10 ** d, 10 ** (d + 1) - 1 if d < 19 else 2 ** 64 - 2)]
assert sorted({len(str(x)) for x in SPECIAL}) == list(range(1, 21)) and len(set(SPECIAL)) == len(SPECIAL)


def regular(rng, n):
    """n floats drawn from every regular exponent (biased 63 .. 158), both signs, as test_pred_text's test_every_regular_exponent"""
    e = (np.arange(n) % 96 + 63).astype(np.uint32)
    rng.shuffle(e)
    frac = rng.integers(0, 1 << 23, n).astype(np.uint32)
    frac[rng.random(n) < 0.1] = 0
    frac[rng.random(n) < 0.05] = 0x7FFFFF
    bits = (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31)) | (e << np.uint32(23)) | frac
    return bits.view(np.float32)


def make_model(seed, n, k, skipped=None):
    """n kept entries and some that are skipped, in a random order: feature ids (SPECIAL first), keys = rev(ids), alternating
    has_V, w = 0 with V (kept), w = 0 and w = -0.0 without V (skipped)"""
    rng = np.random.default_rng(seed)
    skipped = n // 7 + 2 if skipped is None else skipped
    m = n + skipped
    ids = list(SPECIAL[:m])
    while len(ids) < m:
        more = (rng.integers(0, 2 ** 63, 2 * m).astype(U64) >> rng.integers(0, 63, 2 * m).astype(U64)) + U64(2)
        ids = list(dict.fromkeys(ids + [int(x) for x in more]))[:m]
    ids = np.array(ids, U64)[rng.permutation(m)]
    has = (np.arange(m) % 2).astype(np.int32)
    w = regular(rng, m)
    w[(np.arange(m) % 5 == 1) & (has == 1)] = 0.0      # kept: it has V
    w[(np.arange(m) % 6 == 3) & (has == 1)] = -0.0
    if n == 1:
        has[:] = 0   # one kept line, and the skipped ones have no V
    drop = rng.permutation(np.flatnonzero(has == 0) if n > 1 else np.arange(1, m))[:skipped]
    assert drop.size == skipped
    w[drop[0::2]] = 0.0
    w[drop[1::2]] = -0.0
    V = regular(rng, m * k).reshape(m, k) if k else None
    if k:
        V[rng.random((m, k)) < 0.05] = 0.0
    keep = np.ones(m, bool)
    keep[drop] = False
    assert keep.sum() == n
    scal = np.zeros((m, 4), np.float32)
    scal[:, 1] = w
    scal[:, 0] = rng.integers(0, 9, m)   # optimiser state: not in the text
    scal[:, 2] = rng.random(m)
    V2 = np.concatenate([V, rng.random((m, k)).astype(np.float32)], 1) if k else None
    return dict(ids=ids, keys=rev(ids), scal=scal, has=has, V=V, V2=V2, keep=keep, k=k)


def expected(model, key_mode=False):
    """(lines, printed ids) of the kept entries, ascending in the printed id"""
    printed = model["keys"] if key_mode else model["ids"]
    sel = np.flatnonzero(model["keep"])
    sel = sel[np.argsort(printed[sel], kind="stable")]
    lines = render(printed[sel], model["scal"][sel, 1], model["has"][sel], model["V"][sel] if model["k"] else None)
    return lines, printed[sel], sel


@pytest.fixture(scope="module")
def dev():
    from difacto_amd import build, capi
    build.build_hip()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def load(dev, model, capacity=1 << 13, order=None):
    capi, ctx = dev
    tb = capi.Table(ctx, capacity, V_dim=model["k"], init_mode=capi.INIT_HASH, V_threshold=0, l1=0.0, seed=1)
    o = np.arange(len(model["keys"])) if order is None else order
    tb.import_(model["keys"][o], model["scal"][o], model["has"][o], model["V2"][o] if model["k"] else None)
    return tb


def test_oracle_and_model_are_what_they_claim():
    """(no device) the expected text on a hand-written model, and the mix make_model promises"""
    m = dict(ids=np.array([10, 9, 3], U64), keys=rev([10, 9, 3]), scal=np.array([[0, .5, 0, 0], [0, 0, 0, 0], [0, -0.0, 0, 0]], np.float32),
             has=np.array([0, 1, 0], np.int32), V=np.array([[1, 2], [0.25, -3], [7, 7]], np.float32), keep=np.array([True, True, False]), k=2)
    assert b"".join(expected(m)[0]) == b"9\t0\t0.25\t-3\n10\t0.5\n"
    assert int(rev([1])[0]) == 1 << 60 and int(rev(rev([0x0123456789ABCDEF]))[0]) == 0x0123456789ABCDEF
    m = make_model(3, 200, 4)
    kept = m["keep"]
    w = m["scal"][:, 1]
    assert ((w == 0) & (m["has"] == 1) & kept).sum() > 10 and ((w == 0) & ~kept).sum() == (~kept).sum() > 10
    assert np.signbit(w[~kept]).any() and not np.signbit(w[~kept]).all() and (m["has"][~kept] == 0).all()
    assert sorted({len(str(int(i))) for i in m["ids"][kept]}) == list(range(1, 21))
    assert max(len(x) for x in expected(m)[0]) <= 20 + 16 * 5 + 1


V_DIMS = [0, 1, 9, 63, 64, 100, 127]


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("k", V_DIMS)
def test_shapes(dev, k, which):
    capi, ctx = dev
    probe = load(dev, make_model(1, 1, k), capacity=1024)
    d = capi.ModelDump(probe)
    T = d.tile
    d.close()
    probe.close()
    assert T == min(1024, 32768 // (20 + 16 * (1 + k) + 1)) and T >= 15
    n = [1, T - 1, T, T + 1, 3 * T + 5][which]
    model = make_model(100 * k + which, n, k)
    want, ids, _ = expected(model)
    tb = load(dev, model)
    d = capi.ModelDump(tb)
    try:
        assert (d.n, d.tile) == (n, T) and d.shape() == (n, int(model["has"][model["keep"]].sum()), k)
        got, irregular = d.format()
        assert irregular == 0
        assert got.split(b"\n")[:-1] == [x[:-1] for x in want]
        assert got == b"".join(want)
        printed = [int(x.split(b"\t")[0]) for x in got.split(b"\n")[:-1]]
        assert printed == sorted(printed) == [int(i) for i in ids]
    finally:
        d.close()
        tb.close()


@pytest.mark.parametrize("k", [0, 9, 64])
def test_key_mode_same_entries_in_key_order(dev, k):
    capi, ctx = dev
    model = make_model(7 + k, 300, k)
    tb = load(dev, model)
    d = capi.ModelDump(tb, capi.DUMP_IDS_KEY)
    f = capi.ModelDump(tb, capi.DUMP_IDS_FEATURE)
    try:
        want, keys, _ = expected(model, key_mode=True)
        got, irregular = d.format()
        assert irregular == 0 and got == b"".join(want)
        printed = np.array([int(x.split(b"\t")[0]) for x in got.split(b"\n")[:-1]], U64)
        assert np.array_equal(printed, np.sort(model["keys"][model["keep"]]))
        # the same entries as the feature dump's: line for line once the ids are mapped
        ftext, _ = f.format()
        by_id = {int(rev([int(x.split(b"\t")[0])])[0]): x.split(b"\t", 1)[1] for x in ftext.split(b"\n")[:-1]}
        assert by_id == {int(x.split(b"\t")[0]): x.split(b"\t", 1)[1] for x in got.split(b"\n")[:-1]}
    finally:
        d.close()
        f.close()
        tb.close()


@pytest.mark.parametrize("key_mode", [False, True])
def test_bytes_are_a_function_of_the_model_alone(dev, key_mode):
    """two import orders, two capacities (other hash slots, other row numbers): identical bytes"""
    capi, ctx = dev
    model = make_model(11, 700, 9)
    m = len(model["keys"])
    a = load(dev, model, capacity=1 << 11)
    b = load(dev, model, capacity=1 << 15, order=np.random.default_rng(5).permutation(m))
    mode = capi.DUMP_IDS_KEY if key_mode else capi.DUMP_IDS_FEATURE
    da, db = capi.ModelDump(a, mode), capi.ModelDump(b, mode)
    try:
        ta, tb_ = da.format(), db.format()
        assert ta == tb_ and ta[1] == 0 and ta[0] == b"".join(expected(model, key_mode)[0])
        ea, eb = da.entries(), db.entries()
        assert all(np.array_equal(ea[x], eb[x]) for x in ("ids", "w", "has_V", "V"))
    finally:
        for o in (da, db, a, b):
            o.close()


@pytest.mark.parametrize("k", [1, 64])
def test_units_concatenate(dev, k):
    capi, ctx = dev
    probe = load(dev, make_model(1, 1, k), capacity=1024)
    d = capi.ModelDump(probe)
    T = d.tile
    d.close()
    probe.close()
    n = 3 * T + 5
    model = make_model(23 + k, n, k)
    want = expected(model)[0]
    tb = load(dev, model)
    d = capi.ModelDump(tb)
    try:
        whole, irregular = d.format()
        assert irregular == 0 and whole == b"".join(want)
        for cuts in ([0, T // 2, T // 2 + 1, T + 3, 2 * T, 3 * T + 4, n],       # mid-tile, a unit of 1, past a tile edge, a last unit of 1
                     [0, 1, T - 1, T, T + 1, n], [0, 7, 14, 2 * T + 1, n]):
            parts = []
            for first, end in zip(cuts[:-1], cuts[1:]):
                text, irr = d.format(first, end - first)
                assert irr == 0 and text == b"".join(want[first:end]), (first, end)
                parts.append(text)
            assert b"".join(parts) == whole
        assert d.format(5, 0) == (b"", 0) and d.format(n, 0) == (b"", 0)
    finally:
        d.close()
        tb.close()


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


IRREGULAR = [np.nan, np.inf, -np.inf, float(f32([1])[0]), float(f32([0x807FFFFF])[0]), 2.0 ** -70, -2.0 ** -70, 2.0 ** 33, -3e38,
             float(np.nextafter(np.float32(2.0 ** -64), np.float32(0))), 2.0 ** 32]


@pytest.mark.parametrize("k", [0, 9, 100])
def test_irregular_values_are_counted(dev, k):
    """a unit with values the device does not format reports exactly how many; the unit beside it reports none; the entries of
    that unit come back as Table.export holds them, for the host to format"""
    capi, ctx = dev
    n, U = 120, 40   # three units of 40 entries
    model = make_model(31 + k, n, k, skipped=9)
    _, _, sel = expected(model)
    # into the middle unit: w of some entries, V of others (only where the entry has V: a V without has_V is not printed)
    mid = sel[U:2 * U]
    count = 0
    for j, v in enumerate(IRREGULAR):
        model["scal"][mid[3 * j], 1] = v
        count += 1
        if k:
            withv = [e for e in mid if model["has"][e]]
            model["V"][withv[j], (5 * j) % k] = v
            model["V2"][withv[j], (5 * j) % k] = v
            count += 1
            hidden = [e for e in mid if not model["has"][e]]
            model["V2"][hidden[j], 0] = v   # has_V = 0: never read
    tb = load(dev, model)
    d = capi.ModelDump(tb)
    try:
        assert d.n == n
        want = expected(model)[0]
        for u in (0, 2):
            text, irr = d.format(u * U, U)
            assert irr == 0 and text == b"".join(want[u * U:(u + 1) * U])
        text, irr = d.format(U, U)
        assert (text, irr) == (b"", count)
        assert d.format(U + 3 * 2, 1)[1] == 1 + (0 if not k else sum(1 for j in range(len(IRREGULAR)) if [e for e in mid if model["has"][e]][j] == mid[6]))
        assert d.format(0, n)[1] == count
        # the unit's entries: what Table.export holds for those keys
        ent = d.entries(U, U)
        ex = tb.export()
        at = {int(key): i for i, key in enumerate(ex["keys"])}
        rows = [at[int(rev([int(i)])[0])] for i in ent["ids"]]
        assert np.array_equal(ent["ids"], model["ids"][mid])
        assert np.array_equal(ent["w"].view(np.uint32), ex["scal"][rows, 1].view(np.uint32))
        assert np.array_equal(ent["has_V"], ex["has_V"][rows])
        if k:
            assert np.array_equal(ent["V"].view(np.uint32), ex["V"][rows, :k].view(np.uint32))
            assert (ent["V"][ent["has_V"] == 0] == 0).all()
        # and the host's rendering of them is the expected text of the unit (NaN and inf as the C library prints them)
        assert b"".join(render(ent["ids"], ent["w"], ent["has_V"], ent["V"])) == b"".join(want[U:2 * U])
    finally:
        d.close()
        tb.close()


def test_nothing_kept(dev):
    capi, ctx = dev
    tb = capi.Table(ctx, 1024, V_dim=3, init_mode=capi.INIT_HASH, V_threshold=0, l1=0.0, seed=1)
    d = capi.ModelDump(tb)
    assert (d.n, d.format()) == (0, (b"", 0)) and d.entries()["ids"].size == 0
    d.close()
    tb.import_(np.array([5, 6], U64), np.array([[1, 0, 2, 3], [1, -0.0, 2, 3]], np.float32), np.zeros(2, np.int32), np.ones((2, 6), np.float32))
    d = capi.ModelDump(tb)
    assert (d.n, d.shape(), d.format()) == (0, (0, 0, 3), (b"", 0))
    d.close()
    tb.close()


def test_arguments_are_refused(dev):
    capi, ctx = dev
    C = ctypes
    L = capi.lib()
    tb = load(dev, make_model(2, 10, 2))
    h, n = C.c_void_p(), C.c_uint64(0)

    def refused(rc, code, *words):
        msg = L.dfh_last_error().decode()
        assert rc == code and all(x in msg for x in words), (rc, msg)

    refused(L.dfh_dump_open(None, 0, C.byref(h), C.byref(n)), ERR_ARG, "dfh_dump_open", "NULL argument")
    refused(L.dfh_dump_open(tb.h, 0, None, C.byref(n)), ERR_ARG, "dfh_dump_open", "NULL argument")
    refused(L.dfh_dump_open(tb.h, 0, C.byref(h), None), ERR_ARG, "dfh_dump_open", "NULL argument")
    refused(L.dfh_dump_open(tb.h, 2, C.byref(h), C.byref(n)), ERR_ARG, "dfh_dump_open", "ids_mode")
    d = capi.ModelDump(tb)
    nb, irr = C.c_size_t(0), C.c_uint64(0)
    buf = C.create_string_buffer(4096)
    refused(L.dfh_dump_read(d.h, buf), ERR_STATE, "dfh_dump_read", "nothing formatted")
    refused(L.dfh_dump_read(None, buf), ERR_ARG, "dfh_dump_read", "NULL argument")
    refused(L.dfh_dump_format(None, 0, 1, C.byref(nb), C.byref(irr)), ERR_ARG, "dfh_dump_format", "NULL argument")
    refused(L.dfh_dump_format(d.h, 0, 1, None, C.byref(irr)), ERR_ARG, "dfh_dump_format", "NULL argument")
    refused(L.dfh_dump_format(d.h, 0, 1, C.byref(nb), None), ERR_ARG, "dfh_dump_format", "NULL argument")
    for first, count in ((0, 11), (10, 1), (11, 0), (5, 6), (2 ** 64 - 1, 2)):
        refused(L.dfh_dump_format(d.h, first, count, C.byref(nb), C.byref(irr)), ERR_ARG, "dfh_dump_format", "first + count exceeds")
        refused(L.dfh_dump_entries(d.h, first, count, buf, buf, buf, buf), ERR_ARG, "dfh_dump_entries", "first + count exceeds")
    refused(L.dfh_dump_entries(None, 0, 1, buf, buf, buf, buf), ERR_ARG, "dfh_dump_entries", "NULL argument")
    for args in ((None, buf, buf, buf), (buf, None, buf, buf), (buf, buf, None, buf), (buf, buf, buf, None)):
        refused(L.dfh_dump_entries(d.h, 0, 1, *args), ERR_ARG, "dfh_dump_entries", "NULL argument")
    refused(L.dfh_dump_shape(None, None, None, None), ERR_ARG, "dfh_dump_shape", "NULL argument")
    assert L.dfh_dump_tile(None) == 0 and L.dfh_dump_close(None) == 0
    assert d.format()[1] == 0 and d.format(0, 10)[0].count(b"\n") == 10   # still usable
    d.close()
    tb.close()
