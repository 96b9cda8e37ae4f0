"""task = convert with shuffle_rows / shuffle_seed / val_fraction / data_val_out (host/converter.h): the rows of the whole input
go through one row store in HBM and come out in the store's order, split into a training and a validation file.  No GPU: what
Init refuses before the device is touched.  GPU: the written files against numpy's permutation of the host-parsed rows."""
import os
import re

import numpy as np
import pytest

from test_convert_cli import DATA, _criteo_rows, _difacto, built, ing, read_all  # noqa: F401  (fixtures)
from test_rowstore import want_order

N = 1500


# ---------------------------------------------------------------------------------------------------------------------
# no GPU: refused in Init
# ---------------------------------------------------------------------------------------------------------------------
def _convert(built, tmp_path, *args):  # noqa: F811
    return _difacto(built, "task=convert", "data_format=libsvm", "data_out=%s" % (tmp_path / "o"), "data_out_format=rec", *args)


@pytest.mark.parametrize("value", ["2", "-1"])
def test_other_shuffle_rows_is_fatal(built, tmp_path, value):  # noqa: F811
    r = _convert(built, tmp_path, "shuffle_rows=" + value)
    assert r.returncode != 0 and "shuffle_rows=" + value in r.stderr and "0 (file order, the default) and 1" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "o").exists()


@pytest.mark.parametrize("value", ["1", "-0.1", "1.5"])
def test_val_fraction_outside_the_range_is_fatal(built, tmp_path, value):  # noqa: F811
    r = _convert(built, tmp_path, "val_fraction=" + value, "data_val_out=%s" % (tmp_path / "v"))
    assert r.returncode != 0 and "val_fraction=" in r.stderr and "[0, 1)" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "o").exists() and not (tmp_path / "v").exists()


def test_val_fraction_needs_data_val_out(built, tmp_path):  # noqa: F811
    r = _convert(built, tmp_path, "val_fraction=0.2")
    assert r.returncode != 0 and "val_fraction=0.2 needs data_val_out" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "o").exists()


def test_data_val_out_needs_val_fraction(built, tmp_path):  # noqa: F811
    r = _convert(built, tmp_path, "data_val_out=%s" % (tmp_path / "v"), "shuffle_rows=1")
    assert r.returncode != 0 and "data_val_out=" in r.stderr and "with val_fraction=0" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "o").exists() and not (tmp_path / "v").exists()


def test_the_two_outputs_are_different_files(built, tmp_path):  # noqa: F811
    r = _convert(built, tmp_path, "val_fraction=0.5", "data_val_out=%s" % (tmp_path / "o"))
    assert r.returncode != 0 and "data_val_out and data_out are the same file" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "o").exists()


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
class Parsed:
    """the rows of a file as the product's reader gives them"""

    def __init__(self, L, path, fmt):
        off, lab, idx, val, n = read_all(L, path, fmt)
        self.off = np.frombuffer(off, np.uint64).astype(np.int64)
        self.lab, self.idx, self.val, self.n = np.frombuffer(lab, np.float32), np.frombuffer(idx, np.uint64), np.frombuffer(val, np.float32), n

    def rows(self, order):
        """(lengths, labels, ids, values) of these rows in this order"""
        lens = np.diff(self.off)[order]
        take = np.concatenate([np.arange(self.off[r], self.off[r + 1]) for r in order] + [np.zeros(0, np.int64)]).astype(np.int64)
        return lens.tobytes(), self.lab[order].tobytes(), self.idx[take].tobytes(), self.val[take].tobytes()

    def all(self):
        return self.rows(np.arange(self.n))


@pytest.fixture(scope="module")
def text(tmp_path_factory, ing):  # noqa: F811
    """1 500 generated criteo rows, one of them CRLF: its chunk falls back to the host parser under text_parse = device"""
    d = tmp_path_factory.mktemp("criteo_shuffle")
    rows = _criteo_rows(np.random.default_rng(17), N)
    rows[700] = rows[700][:-1] + b"\r\n"
    path = d / "in.txt"
    path.write_bytes(b"".join(rows))
    return str(path), Parsed(ing, path, "criteo"), d


def convert(built, src, out, *args, fmt="criteo", slab="4096"):  # noqa: F811
    env = dict(os.environ, DIFACTO_CHUNK_BYTES="4096", DIFACTO_SLAB_BYTES=slab)
    r = _difacto(built, "task=convert", "data_format=" + fmt, "data_out=%s" % out, "data_out_format=rec", *args, env=env, data=src)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def record_rows(log):
    """rows per record, per output file, from the cumulative `written N examples` lines"""
    files, cur = [], None
    for line in log.splitlines():
        if "writing data to " in line:
            cur = []
            files.append(cur)
        m = re.search(r"written (\d+) examples in", line)
        if m:
            cur.append(int(m.group(1)))
    return [list(np.diff([0] + f)) for f in files]


@pytest.fixture(scope="module")
def plain(built, text):  # noqa: F811
    """the conversion without any of the new keys: (bytes, log, its number of records = the input's non-empty chunks)"""
    src, _, d = text
    log = convert(built, src, d / "plain.rec")
    return (d / "plain.rec").read_bytes(), log, len(record_rows(log)[0])


@pytest.fixture(scope="module")
def shuffled(built, text):  # noqa: F811
    src, _, d = text
    out = {}
    for mode in ("host", "device"):
        log = convert(built, src, d / ("shuf_%s.rec" % mode), "shuffle_rows=1", "shuffle_seed=7", "text_parse=" + mode)
        out[mode] = ((d / ("shuf_%s.rec" % mode)).read_bytes(), log)
    return out


@pytest.mark.gpu
def test_the_default_is_unchanged(built, ing, text, plain):  # noqa: F811
    src, parsed, d = text
    data, log, chunks = plain
    assert chunks > 50 and "rows in HBM" not in log
    assert Parsed(ing, d / "plain.rec", "rec").all() == parsed.all()
    again = convert(built, src, d / "plain2.rec", "shuffle_rows=0", "val_fraction=0", "shuffle_seed=5")
    assert (d / "plain2.rec").read_bytes() == data and "rows in HBM" not in again
    assert record_rows(again) == record_rows(log)


@pytest.mark.gpu
def test_shuffled_output(ing, text, plain, shuffled):  # noqa: F811
    _, parsed, d = text
    (host, host_log), (dev, dev_log) = shuffled["host"], shuffled["device"]
    assert len(host) > 50000 and host == dev
    assert "1 fell back to the host parser" in dev_log and "text_parse" not in host_log
    order = want_order(N, 1, 7)
    assert Parsed(ing, d / "shuf_host.rec", "rec").all() == parsed.rows(order)
    assert parsed.rows(order) != parsed.all()
    R = -(-N // plain[2])
    for log in (host_log, dev_log):
        counts = record_rows(log)
        assert len(counts) == 1 and counts[0] == [R] * (N // R) + ([N % R] if N % R else [])
        m = re.search(r"ordered (\d+) rows in HBM \((\d+) bytes\): (\d+) training and (\d+) validation rows, records of (\d+) rows, "
                      r"shuffle_rows=1 shuffle_seed=7", log)
        assert m, log[-3000:]
        assert [int(x) for x in m.groups()] == [N, int(m.group(2)), N, 0, R] and int(m.group(2)) > len(parsed.idx) * 8


@pytest.mark.gpu
def test_seeds(built, text, shuffled):  # noqa: F811
    src, _, d = text
    convert(built, src, d / "seed8.rec", "shuffle_rows=1", "shuffle_seed=8")
    convert(built, src, d / "seed7.rec", "shuffle_rows=1", "shuffle_seed=7", slab="65536")
    assert (d / "seed8.rec").read_bytes() != shuffled["host"][0]
    assert (d / "seed7.rec").read_bytes() == shuffled["host"][0]


@pytest.mark.gpu
@pytest.mark.parametrize("shuffle", [0, 1])
def test_split(built, ing, text, plain, shuffle):  # noqa: F811
    src, parsed, d = text
    train, val = d / ("train_%d.rec" % shuffle), d / ("val_%d.rec" % shuffle)
    log = convert(built, src, train, "val_fraction=0.2", "data_val_out=%s" % val, "shuffle_rows=%d" % shuffle, "shuffle_seed=7",
                  "text_parse=device")
    n_val = int(np.floor(0.2 * N))
    order = want_order(N, shuffle, 7)
    a, b = Parsed(ing, train, "rec"), Parsed(ing, val, "rec")
    assert (a.n, b.n) == (N - n_val, n_val) == (1200, 300)
    assert a.all() == parsed.rows(order[:N - n_val]) and b.all() == parsed.rows(order[N - n_val:])
    if not shuffle:
        assert b.all() == parsed.rows(np.arange(N - n_val, N))
    R = -(-N // plain[2])
    cut = lambda n: [R] * (n // R) + ([n % R] if n % R else [])   # noqa: E731
    assert record_rows(log) == [cut(N - n_val), cut(n_val)]
    assert "%d training and %d validation rows" % (N - n_val, n_val) in log


@pytest.mark.gpu
def test_parts_of_the_training_output(built, ing, text):  # noqa: F811
    """part_size = 0: a new part after every record (a part holds at least 0 MB), the validation output stays one file"""
    src, parsed, d = text
    out = d / "parts"
    out.mkdir()
    log = convert(built, src, out / "t", "shuffle_rows=1", "shuffle_seed=7", "val_fraction=0.1", "data_val_out=%s" % (out / "v"), "part_size=0")
    names = sorted((p.name for p in out.iterdir()), key=lambda s: (len(s), s))
    counts = record_rows(log)
    assert names == ["v"] + ["t-part_%d" % i for i in range(len(names) - 1)] and len(names) - 1 == len(counts) - 1 > 3
    assert all(len(c) == 1 for c in counts[:-1])
    order = want_order(N, 1, 7)
    got = [Parsed(ing, out / ("t-part_%d" % i), "rec") for i in range(len(names) - 1)]
    want = parsed.rows(order[:N - 150])
    for k in range(4):
        assert b"".join(g.all()[k] for g in got) == want[k]
    assert Parsed(ing, out / "v", "rec").all() == parsed.rows(order[N - 150:])


@pytest.mark.gpu
def test_libsvm_in_and_out(built, ing, tmp_path):  # noqa: F811
    """rcv1 carries real values: the text of the permuted rows, label index:value ..., as the unshuffled conversion prints them"""
    plain_out, out, val = tmp_path / "plain.libsvm", tmp_path / "shuf.libsvm", tmp_path / "val.libsvm"
    r = _difacto(built, "task=convert", "data_format=libsvm", "data_out=%s" % plain_out, "data_out_format=libsvm")
    assert r.returncode == 0, r.stderr[-3000:]
    r = _difacto(built, "task=convert", "data_format=libsvm", "data_out=%s" % out, "data_out_format=libsvm", "shuffle_rows=1", "shuffle_seed=3",
                 "val_fraction=0.25", "data_val_out=%s" % val, env=dict(os.environ, DIFACTO_SLAB_BYTES="4096"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = plain_out.read_bytes().splitlines(keepends=True)
    assert len(lines) == 100
    order = want_order(100, 1, 3)
    assert out.read_bytes() == b"".join(lines[r] for r in order[:75])
    assert val.read_bytes() == b"".join(lines[r] for r in order[75:])
    assert Parsed(ing, out, "libsvm").all()[:3] == Parsed(ing, DATA, "libsvm").rows(order[:75])[:3]   # (values went through %g)


@pytest.mark.gpu
def test_training_from_the_pair(built, text, tmp_path):  # noqa: F811
    """one epoch of learner = sgd on the written pair: the whole-set line counts the validation file's rows, a prediction of the
    training file counts its rows"""
    src, _, d = text
    train, val, model = tmp_path / "train.rec", tmp_path / "val.rec", tmp_path / "model"
    convert(built, src, train, "shuffle_rows=1", "shuffle_seed=1", "val_fraction=0.2", "data_val_out=%s" % val, "text_parse=device")
    args = ["data_format=rec", "learner=sgd", "batch_size=100", "V_dim=4", "V_threshold=2", "l1=.1", "lr=.1"]
    r = _difacto(built, "data_val=%s" % val, "exact_metrics=1", "max_num_epochs=1", "num_jobs_per_epoch=1", "stop_rel_objv=0",
                 "stop_val_auc=-1e30", "model_out=%s" % model, *args, data=str(train))
    assert r.returncode == 0, r.stderr[-3000:]
    assert len(re.findall(r" - Training: loss = ", r.stderr)) == 1
    m = re.findall(r" - Validation \(whole set\): rows=(\d+) ", r.stderr)
    assert m == ["300"], r.stderr[-3000:]
    r = _difacto(built, "task=predict", "model_in=%s" % model, "pred_out=%s" % (tmp_path / "pred"), *args, data=str(train))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "predicted 1200 examples of " in r.stderr, r.stderr[-3000:]
