"""task = dump of the command line (host/model_dump.h): model_in as sorted text in dump_out, "<id>\\t<w>[\\t<V_j>]" per entry with
w != 0 or V, formatted on the device a unit of dump_unit_rows entries at a time (csrc/dfh_dumptext.hip).  No GPU: what Init
refuses before the device is touched, each by its text.  GPU: the file against the Python rendering of Table.load + export of
the same model (snprintf through ctypes), parsed back bit for bit, ids that are the data file's; the same bytes under
dump_write = host and dump_unit_rows = 7; the log line's counts; a tiny weight that sends its unit to the host; a learner = bcd
model; a two-part model through its manifest."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
LINE = (r"task=dump dump_write=(\w+): (\d+) entries \((\d+) with V\) to (\S+), (\d+) units / (\d+) entries formatted on the device, "
        r"(\d+) units / (\d+) entries on the host, (\d+) bytes")
U64 = np.uint64
_libc = ctypes.CDLL(None)


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


def _difacto(built, *args, env=None, timeout=300):
    return subprocess.run([os.path.join(built, "difacto")] + list(args), capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)


# ---------------------------------------------------------------------------------------------------------------------
# no GPU: refused in Init, before the device is touched
# ---------------------------------------------------------------------------------------------------------------------
def _refused(r, *words):
    assert r.returncode != 0 and all(w in r.stderr for w in words), r.stderr[-2000:]


def test_no_model_in(built):
    _refused(_difacto(built, "task=dump", "dump_out=none"), "task=dump needs model_in", "the model file")


def test_no_dump_out(built):
    _refused(_difacto(built, "task=dump", "model_in=none"), "task=dump needs dump_out", "the text file to write")


def test_other_dump_ids(built):
    _refused(_difacto(built, "task=dump", "model_in=none", "dump_out=none", "dump_ids=raw"), "dump_ids=raw is not one of feature", "and key")


def test_other_dump_write(built):
    _refused(_difacto(built, "task=dump", "model_in=none", "dump_out=none", "dump_write=gpu"), "dump_write=gpu is not one of device (the default) and host")


@pytest.mark.parametrize("rows", ["0", "-3"])
def test_unit_of_no_rows(built, rows):
    _refused(_difacto(built, "task=dump", "model_in=none", "dump_out=none", "dump_unit_rows=" + rows), "dump_unit_rows=" + rows,
             "a unit has 1 entry or more")


def test_unreadable_model_in(built, tmp_path):
    missing = str(tmp_path / "no_such_model")
    out = str(tmp_path / "out.txt")
    _refused(_difacto(built, "task=dump", "model_in=" + missing, "dump_out=" + out), "cannot read " + missing, missing + ".parts")
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
    bad = tmp_path / "not_a_model"
    bad.write_bytes(b"hello, this is no model file at all")
    _refused(_difacto(built, "task=dump", "model_in=" + str(bad), "dump_out=" + out), str(bad) + " is not a model file")


def test_a_rank_is_refused(built, tmp_path):
    env = dict(os.environ, DMLC_ROLE="worker", DMLC_NUM_WORKER="2", DIFACTO_RANK="0", DIFACTO_DEVICE="0", DIFACTO_COMM="file",
               DIFACTO_RENDEZVOUS=str(tmp_path))
    _refused(_difacto(built, "task=dump", "model_in=none", "dump_out=none", env=env), "task=dump in the environment of a rank", "DMLC_ROLE",
             "through its manifest")


def test_unknown_task_names_dump(built):
    _refused(_difacto(built, "task=export"), "unknown task: export", "train, predict, convert and dump")


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def rev(x):
    """ReverseBytes (include/difacto/base.h): the nibbles of a 64-bit word in reverse order"""
    x = np.asarray(x, U64).byteswap()
    return ((x & U64(0x0F0F0F0F0F0F0F0F)) << U64(4)) | ((x & U64(0xF0F0F0F0F0F0F0F0)) >> U64(4))


def _fmt(spec, arg):
    buf = ctypes.create_string_buffer(40)
    n = _libc.snprintf(buf, 40, spec, arg)
    assert 0 < n < 40
    return buf.raw[:n]


def render(ex, k, key_mode=False):
    """the expected file of an exported table: the keep rule and order of the issue, the C library's formatting"""
    w = ex["scal"][:, 1]
    keep = np.flatnonzero((w != 0) | (ex["has_V"] != 0))
    printed = ex["keys"] if key_mode else rev(ex["keys"])
    keep = keep[np.argsort(printed[keep])]
    out = []
    for i in keep:
        line = _fmt(b"%llu", ctypes.c_ulonglong(int(printed[i]))) + _fmt(b"\t%.9g", ctypes.c_double(float(w[i])))
        if ex["has_V"][i]:
            line += b"".join(_fmt(b"\t%.9g", ctypes.c_double(float(x))) for x in ex["V"][i, :k])
        out.append(line + b"\n")
    return b"".join(out), keep


@pytest.fixture(scope="module")
def dev(built):
    from difacto_amd import capi
    ctx = capi.Context(0)
    yield capi, ctx
    ctx.close()


def exported(dev, path, k):
    capi, ctx = dev
    tb = capi.Table(ctx, 1 << 16, V_dim=k, init_mode=capi.INIT_HASH)
    tb.load(path)
    ex = tb.export()
    tb.close()
    return ex


def _dump(built, model, out, *extra):
    r = _difacto(built, "task=dump", "model_in=" + model, "dump_out=" + out, *extra)
    assert r.returncode == 0, r.stderr[-3000:]
    found = re.findall(LINE, r.stderr)
    assert len(found) == 1, r.stderr[-3000:]
    f = found[0]
    assert not os.path.exists(out + ".tmp")
    text = open(out, "rb").read()
    counts = dict(write=f[0], entries=int(f[1]), with_V=int(f[2]), path=f[3], dev_units=int(f[4]), dev_entries=int(f[5]), host_units=int(f[6]),
                  host_entries=int(f[7]), bytes=int(f[8]))
    assert counts["path"].rstrip(",") == out and counts["bytes"] == len(text) and counts["entries"] == text.count(b"\n")
    assert counts["dev_entries"] + counts["host_entries"] == counts["entries"]
    return counts, text


# (l1 = 0: every feature the training saw has a weight; V_threshold = 2: some entries have V, some do not)
TRAIN = ["data_in=" + DATA, "V_dim=4", "batch_size=10", "max_num_epochs=3", "num_jobs_per_epoch=2", "V_threshold=2", "l1=0", "lr=.05",
         "stop_rel_objv=0", "stop_val_auc=-1e30"]


@pytest.fixture(scope="module")
def model(built, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("dump_cli") / "model")
    r = _difacto(built, "model_out=" + path, *TRAIN)
    assert r.returncode == 0, r.stderr[-3000:]
    return path


@pytest.fixture(scope="module")
def model_text(built, dev, model):
    """the expected file, once"""
    ex = exported(dev, model, 4)
    text, keep = render(ex, 4)
    return ex, keep, text


@pytest.mark.gpu
def test_dump_of_a_trained_model(built, model, model_text, tmp_path):
    ex, keep, want = model_text
    counts, text = _dump(built, model, str(tmp_path / "dump.txt"))
    n_v = int((ex["has_V"][keep] != 0).sum())
    assert keep.size > 100 and 0 < n_v < keep.size, "the model mixes entries with and without V"
    assert counts == dict(counts, write="device", entries=keep.size, with_V=n_v, dev_units=1, dev_entries=keep.size, host_units=0, host_entries=0)
    assert text == want
    # parsed back: the exported w and V bit for bit, in ascending id order, two fields where there is no V
    lines = text.split(b"\n")[:-1]
    ids = np.array([int(l.split(b"\t")[0]) for l in lines], U64)
    assert np.array_equal(ids, np.sort(ids)) and np.array_equal(ids, rev(ex["keys"][keep]))
    for l, i in zip(lines, keep):
        tok = l.split(b"\t")
        assert len(tok) == (2 + 4 if ex["has_V"][i] else 2)
        vals = np.array([float(t) for t in tok[1:]], np.float64).astype(np.float32)
        assert vals[0].view(np.uint32) == ex["scal"][i, 1].view(np.uint32)
        if ex["has_V"][i]:
            assert np.array_equal(vals[1:].view(np.uint32), ex["V"][i, :4].view(np.uint32))
    # dump_ids = feature: every printed id is an id of the data file
    in_file = {int(tok.split(":")[0]) for row in open(DATA) for tok in row.split()[1:]}
    assert {int(i) for i in ids} <= in_file


@pytest.mark.gpu
@pytest.mark.parametrize("extra,units", [(["dump_write=host"], ("host", 1)), (["dump_unit_rows=7"], ("device", None)),
                                         (["dump_write=host", "dump_unit_rows=100"], ("host", None))])
def test_same_bytes(built, model, model_text, tmp_path, extra, units):
    _, keep, want = model_text
    counts, text = _dump(built, model, str(tmp_path / "dump.txt"), *extra)
    assert text == want
    unit = int(([e.split("=")[1] for e in extra if e.startswith("dump_unit_rows=")] or ["65536"])[0])
    n_units = (keep.size + unit - 1) // unit
    where, other = ("host", "dev") if units[0] == "host" else ("dev", "host")
    assert counts["write"] == units[0] and (units[1] is None or units[1] == n_units)
    assert (counts[where + "_units"], counts[where + "_entries"]) == (n_units, keep.size)
    assert (counts[other + "_units"], counts[other + "_entries"]) == (0, 0)


@pytest.mark.gpu
def test_dump_ids_key(built, dev, model, model_text, tmp_path):
    ex, _, feature_text = model_text
    want, keep = render(ex, 4, key_mode=True)
    counts, text = _dump(built, model, str(tmp_path / "dump.txt"), "dump_ids=key")
    assert text == want and text != feature_text
    ids = np.array([int(l.split(b"\t")[0]) for l in text.split(b"\n")[:-1]], U64)
    assert np.array_equal(ids, np.sort(ex["keys"][keep]))


@pytest.mark.gpu
def test_a_tiny_weight_sends_its_unit_to_the_host(built, dev, tmp_path):
    """saved through capi: 35 entries, the 13th id carries |w| < 2^-64; units of 10: the second is the host's, the file is exact"""
    capi, ctx = dev
    k = 3
    rng = np.random.default_rng(4)
    ids = np.arange(1, 36).astype(U64) * U64(1000003)
    scal = np.zeros((35, 4), np.float32)
    scal[:, 1] = rng.normal(size=35)
    scal[12, 1] = 1e-30
    has = (np.arange(35) % 3 != 0).astype(np.int32)
    V = np.concatenate([rng.normal(size=(35, k)), np.zeros((35, k))], 1).astype(np.float32)
    tb = capi.Table(ctx, 1024, V_dim=k, init_mode=capi.INIT_HASH)
    tb.import_(rev(ids), scal, has, V)
    path = str(tmp_path / "tiny.model")
    assert tb.save(path, save_aux=False) == 35
    want, keep = render(tb.export(), k)
    tb.close()
    assert want.count(b"e-30") == 1 and keep.size == 35
    counts, text = _dump(built, path, str(tmp_path / "dump.txt"), "dump_unit_rows=10")
    assert text == want
    assert counts == dict(counts, entries=35, with_V=int(has.sum()), dev_units=3, dev_entries=25, host_units=1, host_entries=10)
    assert [int(l.split(b"\t")[0]) for l in text.split(b"\n")[:-1]] == [int(i) for i in ids]


@pytest.mark.gpu
def test_dump_of_a_bcd_model(built, dev, tmp_path):
    m = str(tmp_path / "m")
    r = _difacto(built, "learner=bcd", "data_in=" + DATA, "max_num_epochs=2", "l1=.1", "lr=.8", "block_ratio=1", "tail_feature_filter=0",
                 "model_out=" + m)
    assert r.returncode == 0, r.stderr[-3000:]
    want, keep = render(exported(dev, m, 0), 0)
    counts, text = _dump(built, m, str(tmp_path / "dump.txt"))
    assert keep.size > 20 and text == want
    assert counts == dict(counts, entries=keep.size, with_V=0, dev_entries=keep.size, host_entries=0)
    assert all(len(l.split(b"\t")) == 2 for l in text.split(b"\n")[:-1])


@pytest.mark.gpu
def test_two_parts_through_the_manifest(built, dev, tmp_path):
    """two tables saved as <m>.part-0 and <m>.part-1, the manifest written by hand: the dump of <m> is the dump of the merged table"""
    capi, ctx = dev
    k = 2
    rng = np.random.default_rng(8)
    ids = np.unique(rng.integers(1, 1 << 50, 400).astype(U64))[:300]
    keys = rev(ids)
    scal = np.zeros((300, 4), np.float32)
    scal[:, 1] = rng.normal(size=300) * 10.0 ** rng.integers(-5, 6, 300)
    has = (rng.random(300) < 0.5).astype(np.int32)
    V = np.concatenate([rng.normal(size=(300, k)), np.zeros((300, k))], 1).astype(np.float32)
    lo = keys < np.median(keys)   # a sharded save splits by key range
    name = str(tmp_path / "sharded")
    tables = []
    for part, sel in enumerate((lo, ~lo)):
        tb = capi.Table(ctx, 1024, V_dim=k, init_mode=capi.INIT_HASH)
        tb.import_(keys[sel], scal[sel], has[sel], V[sel])
        assert tb.save("%s.part-%d" % (name, part), save_aux=bool(part)) == int(sel.sum())   # (optimiser state in a part is left behind)
        tables.append(tb)
    with open(name + ".parts", "w") as f:
        f.write("2\n")
    merged = capi.Table(ctx, 1024, V_dim=k, init_mode=capi.INIT_HASH)
    merged.import_(keys, scal, has, V)
    single = str(tmp_path / "single.model")
    assert merged.save(single, save_aux=False) == 300
    want, keep = render(merged.export(), k)
    for tb in tables + [merged]:
        tb.close()
    assert keep.size == 300
    _, from_parts = _dump(built, name, str(tmp_path / "parts.txt"), "dump_unit_rows=64")
    _, from_single = _dump(built, single, str(tmp_path / "single.txt"))
    assert from_parts == from_single == want
