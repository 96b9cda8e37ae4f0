"""The device prediction text (csrc/dfh_predtext.hip, csrc/dfh_predtext_fmt.h) through capi.PredText: the bytes of
fprintf("%.9g\\n", v) for every appended value, against the C library itself (snprintf through ctypes: what the host path of
task = predict uses).  Text must be EQUAL, byte for byte.

The device formats the regular values (+-0 and 2^-64 <= |v| < 2^32) and counts the others.  A tile of the two format kernels
is PredText.TILE values (256 lanes x 4 rounds); a tile's text starts at whatever byte the tile before it ends, the aligned
16 B words in between are written as vectors and the unaligned head and tail byte by byte, so the sizes sit on one wave, one
tile and several tiles with lines of every length 2 .. 16."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_libc = ctypes.CDLL(None)


def line(v):
    """the oracle: what fprintf("%.9g\\n", v) writes for the float v"""
    buf = ctypes.create_string_buffer(32)
    n = _libc.snprintf(buf, 32, b"%.9g\n", ctypes.c_double(float(v)))
    assert 0 < n < 32
    return buf.raw[:n]


def text(vals):
    return b"".join(line(v) for v in np.asarray(vals, np.float32))


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def dev():
    from difacto_amd import build, capi
    build.build_hip()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def fmt(dev, vals, hint=0):
    capi, ctx = dev
    p = capi.PredText(ctx, hint)
    try:
        p.append_host(np.asarray(vals, np.float32))
        return p.format()
    finally:
        p.close()


def test_every_regular_exponent(dev):
    rng = np.random.default_rng(5)
    bits = [0x00000000, 0x80000000]
    for e in range(63, 159):
        fracs = [0, 1, 0x400000, 0x7FFFFF] + [int(x) for x in rng.integers(0, 1 << 23, 4)]
        for s in (0, 1):
            bits += [s << 31 | e << 23 | f for f in fracs]
    vals = f32(bits)
    assert vals.size == 2 + 96 * 16 and np.abs(vals[2:]).min() == 2.0 ** -64 and np.abs(vals).max() < 2.0 ** 32
    want = [line(v) for v in vals]
    assert max(len(w) for w in want) <= 16
    got, irregular = fmt(dev, vals)
    assert irregular == 0
    assert got.split(b"\n")[:-1] == [w[:-1] for w in want]
    assert got == b"".join(want)


SIG20 = np.float32(1.0) / (np.float32(1.0) + np.exp(np.float32(-20.0)))
SIGM20 = np.float32(1.0) / (np.float32(1.0) + np.exp(np.float32(20.0)))
DESIGNED = [
    (2097151.875, b"2097151.88"), (2097151.625, b"2097151.62"), (2097151.375, None), (1048575.9375, None),   # exact ties
    (0.5, b"0.5"), (16.0, b"16"), (1e8, b"100000000"), (1e9, b"1e+09"), (123456792.0, b"123456792"), (999999936.0, b"999999936"),
    (4294967040.0, None), (2.0 ** -64, b"5.42101086e-20"),
    (1e-4, b"9.99999975e-05"),                                       # scientific goes by the ROUNDED exponent
    (float(np.nextafter(np.float32(1e-4), np.float32(1))), None),   # fixed: 0.000100000005
    (0.001, None), (20.0, b"20"), (-20.0, b"-20"), (float(SIG20), None), (float(SIGM20), None),
]


def test_designed_values_are_what_they_claim():
    """(no device) the oracle on the designed values: the expected strings, and the lengths the file's head speaks of"""
    for v, s in DESIGNED:
        assert float(np.float32(v)) == v or v in (1e-4, 0.001), v   # exactly floats (but the two decimal literals)
        if s is not None:
            assert line(np.float32(v)) == s + b"\n", (v, line(np.float32(v)))
    up = float(np.nextafter(np.float32(1e-4), np.float32(1)))
    assert b"e" not in line(up) and len(line(-up)) == 16
    assert line(SIGM20).startswith(b"2.06") and b"e-09" in line(SIGM20)


@pytest.mark.parametrize("k", range(len(DESIGNED)))
def test_designed_value_alone(dev, k):
    for v in (DESIGNED[k][0], -DESIGNED[k][0]):
        got, irregular = fmt(dev, [v])
        assert (got, irregular) == (line(np.float32(v)), 0), v


def test_designed_values_together(dev):
    vals = np.array([v for v, _ in DESIGNED] + [-v for v, _ in DESIGNED], np.float32)
    got, irregular = fmt(dev, vals)
    assert irregular == 0 and got == text(vals)


# lines of 2 .. 16 bytes with their '\n': the values cycle, so tile boundaries fall on every byte alignment
BY_LENGTH = [0.0, -0.0, -16.0, 1.25, -1.25, -1.125, 12.0625, -12.0625, 123456.75, -123456.75, 0.005859375, -0.005859375,
             -0.0009765625, 1e-4, -1.23456789e-5]
assert len(BY_LENGTH) == 15


def test_by_length_has_every_length():
    assert sorted(len(line(np.float32(v))) for v in BY_LENGTH) == list(range(2, 17))


def _sizes():
    from difacto_amd import capi
    t = capi.PredText.TILE
    return [0, 1, 63, 64, 65, t - 1, t, t + 1, 3 * t + 17]


@pytest.mark.parametrize("which", range(9))
def test_sizes(dev, which):
    n = _sizes()[which]
    vals = np.resize(np.array(BY_LENGTH, np.float32), n) if n else np.zeros(0, np.float32)
    got, irregular = fmt(dev, vals)
    assert irregular == 0
    assert got == text(vals)
    if n == 0:
        assert got == b""


def test_appends_in_pieces_and_reset(dev):
    capi, ctx = dev
    rng = np.random.default_rng(9)
    vals = (rng.normal(size=1064) * 10.0 ** rng.integers(-6, 7, 1064)).astype(np.float32)
    p = capi.PredText(ctx, 16)
    at = 0
    for piece in (1, 0, 63, 1000):
        p.append_host(vals[at:at + piece])
        at += piece
        assert p.count() == at
        got, irregular = p.format()
        assert irregular == 0 and got == text(vals[:at]), piece
    assert at == vals.size and np.array_equal(p.values(), vals)
    p.reset()
    assert p.count() == 0 and p.format() == (b"", 0)
    other = (rng.random(77) * 40 - 20).astype(np.float32)
    p.append_host(other)
    got, irregular = p.format()
    assert irregular == 0 and got == text(other)
    p.close()


IRREGULAR = [float(np.nextafter(np.float32(2.0 ** -64), np.float32(0))), 2.0 ** 32, 3e38, float(f32([1])[0]), math.inf, -math.inf,
             math.nan]


def test_irregular_values_are_counted(dev):
    rng = np.random.default_rng(2)
    regular = (rng.random(200) * 40 - 20).astype(np.float32)
    got, irregular = fmt(dev, regular)
    assert irregular == 0 and got == text(regular)
    for k, v in enumerate(IRREGULAR):
        vals = np.insert(regular, 13 * k, np.float32(v))
        assert fmt(dev, vals)[1] == 1, v
    vals = regular
    for k, v in enumerate(IRREGULAR):
        vals = np.insert(vals, 29 * k, np.float32(v))
    assert fmt(dev, vals)[1] == 7


@pytest.mark.parametrize("with_eval", [False, True])
def test_append_batch(with_eval):
    """the learner's loop: preparation streams on, ONE batch object, load -> localize -> step -> append, reloaded at once with
    nothing read back in between.  The text is that of the predictions a second pass reads after each step"""
    from difacto_amd import capi
    rng = np.random.default_rng(21)
    ctx = capi.Context(0)
    ctx.set_pipeline(2)
    k, U = 4, 300
    ids = np.unique(rng.integers(1, 1 << 40, 2 * U).astype(np.uint64))[:U]   # raw feature ids; the store holds ReverseBytes(id)
    keys = ids.byteswap()
    keys = ((keys & np.uint64(0x0F0F0F0F0F0F0F0F)) << np.uint64(4)) | ((keys & np.uint64(0xF0F0F0F0F0F0F0F0)) >> np.uint64(4))
    order = np.argsort(keys)
    ids, keys = ids[order], keys[order]
    scal = np.stack([rng.integers(0, 5, U), rng.normal(size=U) * 0.3, np.abs(rng.normal(size=U)), rng.normal(size=U) * 0.3],
                    1).astype(np.float32)
    V = np.concatenate([rng.normal(size=(U, k)) * 0.3, np.abs(rng.normal(size=(U, k))) * 0.2], 1).astype(np.float32)
    tb = capi.Table(ctx, 1 << 12, V_dim=k, init_mode=capi.INIT_HASH, V_threshold=0, l1=0.0, seed=1)
    tb.import_(keys, scal, np.ones(U, np.int32), V)
    parts = []
    for nrows in (130, 37):
        off = (np.arange(nrows + 1) * 3).astype(np.uint64)
        idx = ids[rng.integers(0, U, nrows * 3)]
        val = rng.normal(size=nrows * 3).astype(np.float32)
        lab = np.where(rng.random(nrows) < 0.5, 1.0, -1.0).astype(np.float32)
        parts.append((off, idx, val, lab))
    b = capi.Batch(ctx, 130, 130 * 3)
    p = capi.PredText(ctx, 16)
    e = capi.Eval(ctx, 16) if with_eval else None
    for part in parts:
        b.load_host(*part)
        b.localize()
        b.sgd_step(tb, is_train=False)
        if e:
            e.append_batch(b)
        p.append_batch(b)
    got, irregular = p.format()
    preds = []
    for part in parts:
        b.load_host(*part)
        b.localize()
        b.sgd_step(tb, is_train=False)
        preds.append(b.pred())
    assert np.unique(np.concatenate(preds)).size > 100
    assert irregular == 0 and p.count() == 167
    assert got == text(np.concatenate(preds))
    if e:
        r = e.finish()
        assert r.n == 167 and r.n_pos == int(sum((q[3] > 0).sum() for q in parts))
        e.close()
    for o in (p, b, tb):
        o.close()
    ctx.close()
