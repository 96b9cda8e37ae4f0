"""The lines of explain_out and recommend_out formatted on the device (csrc/dfh_listtext.hip) through capi.Explain.format /
capi.Recommend.format, byte for byte against plain Python over what read() returns: "%.9g" of inter, "\\t%d:%d:%.9g" per pair;
"%d:%.9g" joined by tabs.  Row counts T + 1 and 2 T + 3 (T = text_tile: a full tile, a partial one, tiles that start off a
16 B word); lists of 0, 1 and K entries in one unit; designed tokens; a float below 2^-64 is reported, not formatted."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U64, F32 = np.uint64, np.float32
ERR_STATE = 4   # DFH_ERR_STATE of include/difacto_hip.h


def rev(x):   # ReverseBytes (include/difacto/base.h)
    x = np.asarray(x, U64).byteswap()
    return ((x & U64(0x0F0F0F0F0F0F0F0F)) << U64(4)) | ((x & U64(0xF0F0F0F0F0F0F0F0)) >> U64(4))


@pytest.fixture(scope="module")
def dev():
    from difacto_amd import build, capi
    build.build_hip()
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def g9(v):
    return "%.9g" % float(F32(v))


def explain_text(got):
    return "".join(g9(got["inter"][r]) + "".join("\t%d:%d:%s" % (got["ids_i"][r, j], got["ids_j"][r, j], g9(got["c"][r, j]))
                                                  for j in range(got["n"][r])) + "\n" for r in range(len(got["n"]))).encode()


def recommend_text(got):
    return "".join("\t".join("%d:%s" % (got["items"][q, j], g9(got["logits"][q, j])) for j in range(got["n"][q])) + "\n"
                   for q in range(len(got["n"]))).encode()


def table(dev, ids, w, has, V):
    capi, ctx = dev
    scal = np.zeros((len(ids), 4), F32)
    scal[:, 1] = w
    tb = capi.Table(ctx, 1024, V_dim=V.shape[1], init_mode=capi.INIT_HASH, V_threshold=0, l1=0.0, seed=1)
    tb.import_(rev(ids), scal, np.asarray(has, np.int32), np.concatenate([V, np.zeros_like(V)], 1).astype(F32))
    return tb


def stepped(dev, tb, ids, lens, idx, x):
    capi, ctx = dev
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    b = capi.Batch(ctx, len(lens), max(int(off[-1]), 1))
    b.load_host(off, ids[idx], np.asarray(x, F32), np.ones(len(lens), F32))
    b.localize()
    b.lookup(tb)
    b.sgd_step(tb, is_train=False)
    return b


def random_model(dev, seed, m=40, k=4):
    rng = np.random.default_rng(seed)
    ids = np.arange(1, m + 1, dtype=U64) * U64(7919)
    return table(dev, ids, rng.normal(size=m), np.ones(m), rng.normal(size=(m, k))), ids


def rows(rng, ids, R):
    """row lengths 0 .. 12 going round, every key with V: rows of 0, 0, 1, 3, .. 66 pairs in one unit"""
    lens = np.arange(R) % 13
    return lens, rng.integers(0, len(ids), lens.sum()), rng.normal(size=lens.sum())


@pytest.mark.parametrize("K", [1, 10, 32])
def test_explain_layout(dev, K):
    capi, ctx = dev
    tb, ids = random_model(dev, K)
    e = capi.Explain(ctx, K)
    T = e.text_tile
    assert T == min(1024, 32768 // (15 + 58 * K + 1))
    rng = np.random.default_rng(K + 1)
    seen = set()
    for R in (T + 1, 2 * T + 3):   # the second unit, behind a reset, does not depend on the first
        e.reset()
        b = stepped(dev, tb, ids, *rows(rng, ids, R))
        e.append_batch(b, tb)
        text, irr = e.format()
        got = e.read()   # stays valid beside a format
        seen |= set(got["n"].tolist())
        assert irr == 0 and e.text_nonfinite() == 0 and text == explain_text(got) and text.count(b"\n") == R
        b.close()
    assert {0, 1, K} <= seen and b"\n0\n" in text
    e.close(), tb.close()


@pytest.mark.parametrize("K", [1, 10, 32])
def test_recommend_layout(dev, K):
    capi, ctx = dev
    tb, ids = random_model(dev, 50 + K)
    rng = np.random.default_rng(K + 2)
    r = capi.Recommend(ctx, K)
    T = r.text_tile
    assert T == min(1024, 32768 // (27 * K + 1))
    for M, R in ((max(K // 2, 1), T + 1), (K + 5, 2 * T + 3)):   # M < K: short lists; then full ones, the catalogue grown
        r.reset()
        b = stepped(dev, tb, ids, *rows(rng, ids, M - r.item_count()))
        r.add_items(b, tb)
        b.close()
        b = stepped(dev, tb, ids, *rows(rng, ids, R))
        r.append_batch(b, tb)
        text, irr = r.format()
        got = r.read()
        assert irr == 0 and (got["n"] == min(M, K)).all() and text == recommend_text(got) and text.count(b"\n") == R
        b.close()
    r.close(), tb.close()


def test_tokens(dev):
    """ids of 1 and 20 digits; items 0 and 10^6; floats 0, negative, nine digits, exponent form, at or above 1e9 and below 2^32 (2e+09)
    (a sum that starts at +0 never gives -0: that token is tools/list_fmt_check.cc's)"""
    capi, ctx = dev
    ids = np.array([3, 7, 10 ** 19 + 11, 18446744073709551557, 42, 12345678901234567890], U64)
    V = np.array([[1, 0], [-1, 0], [0, 1.23456789], [0, 1e-3], [40000, 0], [50000, 0.5]], F32)
    tb = table(dev, ids, [0.5, -0.25, 1e-5, 0, 3, -2], np.ones(6), V)
    b = stepped(dev, tb, ids, [2, 3, 2, 2, 6, 1, 0], [0, 2, 0, 1, 3, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5, 4],
                [1, 1, 1, 1, 1, 1, 1e-3, 1, 1, 1, 1, 3, 1, 1, 1, 1])
    e = capi.Explain(ctx, 10)
    e.append_batch(b, tb)
    text, irr = e.format()
    assert irr == 0 and text == explain_text(e.read())
    for tok in (b"\t3:10000000000000000011:0", b"e-0", b"\t3:7:-1", b"\t42:12345678901234567890:2e+09", b":0.0037037", b"\n0\n"):
        assert tok in text, tok
    # the catalogue: 10^6 + 1 rows, empty but for the first and the last, whose b = 1 + 2e9 ranks them first: items 0 and 10^6
    M = 10 ** 6 + 1
    r = capi.Recommend(ctx, 3, capacity_hint=M)
    cl = np.zeros(M, np.int64)
    cl[0] = cl[-1] = 2
    bi = stepped(dev, tb, ids, cl, [4, 5, 4, 5], [1, 1, 1, 1])
    r.add_items(bi, tb)
    bq = stepped(dev, tb, ids, [2, 1, 0], [0, 2, 1], [1, 1, 1])
    r.append_batch(bq, tb)
    text, irr = r.format()
    got = r.read()
    assert irr == 0 and text == recommend_text(got)
    assert got["items"].tolist() == [[0, 10 ** 6, 1]] * 3 and text.endswith(b"0:2e+09\t1000000:2e+09\t1:0\n")
    for o in (r, e, b, bi, bq, tb):
        o.close()


def test_irregular_and_state(dev):
    capi, ctx = dev
    L = capi.lib()
    ids = np.array([3, 7, 11], U64)
    tb = table(dev, ids, [1, 1, 1], np.ones(3), np.array([[1, 0], [2, 0], [1e-12, 0]], F32))
    buf = ctypes.create_string_buffer(4096)
    for with_tiny, want in ((True, 1), (False, 0)):
        e, r = capi.Explain(ctx, 10), capi.Recommend(ctx, 2)
        assert L.dfh_explain_read_text(e.h, buf) == ERR_STATE and L.dfh_recommend_read_text(r.h, buf) == ERR_STATE
        # row 1: c = 1e-12 * 1e-12 = 1e-24, nonzero and below 2^-64
        b = stepped(dev, tb, ids, [2, 2] if with_tiny else [2], [0, 1, 2, 2][:4 if with_tiny else 2], [1.0] * (4 if with_tiny else 2))
        e.append_batch(b, tb)
        text, irr = e.format()
        assert (irr >= 1) == bool(want) and text == (b"" if want else explain_text(e.read()))
        if not want:
            assert text == b"2\t3:7:2\n" and L.dfh_explain_read_text(e.h, buf) == 0
        e.append_batch(b, tb)
        assert L.dfh_explain_read_text(e.h, buf) == ERR_STATE and "format" in L.dfh_last_error().decode()
        r.add_items(b, tb)
        r.append_batch(b, tb)
        text, irr = r.format()
        assert irr == 0 and text == recommend_text(r.read())
        r.append_batch(b, tb)
        assert L.dfh_recommend_read_text(r.h, buf) == ERR_STATE
        r.reset()
        assert r.format() == (b"", 0)
        for o in (e, r, b):
            o.close()
    tb.close()
