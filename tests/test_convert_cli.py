"""task = convert of the command line (host/converter.h): data_in -> libsvm text or a .rec file whose row blocks are compressed
on the device.  No GPU: what Init refuses before the device is touched, and the RecordIO writer (host/recordio_writer.h through
ingest_write_recordio) against oracle.ingest.write_recordio.  GPU: criteo -> rec with the text parsed on the host and on the
device, training from the converted file, parts, libsvm -> rec -> rec -> libsvm."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
MAGIC = struct.pack("<I", 0xced7230a)


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


@pytest.fixture(scope="module")
def ing(built):
    L = C.CDLL(os.path.join(built, "libdifacto_ingest.so"))
    L.ingest_write_recordio.restype = C.c_long
    L.ingest_write_recordio.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.ingest_read.restype = C.c_long
    L.ingest_read.argtypes = [C.c_char_p, C.c_char_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_size_t, C.c_size_t,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_long)]
    return L


def _difacto(built, *args, env=None, data=DATA, timeout=300):
    return subprocess.run([os.path.join(built, "difacto"), "data_in=" + data] + list(args), capture_output=True, text=True, timeout=timeout,
                          cwd=ROOT, env=env)


def read_all(L, path, fmt, cap_rows=50000, cap_nnz=2000000):
    off = np.zeros(cap_rows + 1, np.uint64)
    lab = np.zeros(cap_rows, np.float32)
    idx = np.zeros(cap_nnz, np.uint64)
    val = np.zeros(cap_nnz, np.float32)
    hv, nb = C.c_int(0), C.c_long(0)
    n = L.ingest_read(str(path).encode(), fmt.encode(), 0, 1, 100, 0, 1.0, cap_rows, cap_nnz, off.ctypes.data, lab.ctypes.data,
                      idx.ctypes.data, val.ctypes.data, C.byref(hv), C.byref(nb))
    assert n >= 0
    nnz = int(off[n])
    return off[:n + 1].tobytes(), lab[:n].tobytes(), idx[:nnz].tobytes(), val[:nnz].tobytes(), n


# ---------------------------------------------------------------------------------------------------------------------
# no GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_missing_data_out_is_fatal(built):
    r = _difacto(built, "task=convert", "data_format=libsvm", "data_out_format=rec")
    assert r.returncode != 0 and "data_out" in r.stderr and "unknown task" not in r.stderr, r.stderr[-2000:]


def test_other_output_format_is_fatal(built, tmp_path):
    r = _difacto(built, "task=convert", "data_format=libsvm", "data_out=%s" % (tmp_path / "o"), "data_out_format=parquet")
    assert r.returncode != 0 and "data_out_format=parquet" in r.stderr and "libsvm or rec" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "o").exists()


def test_a_rank_is_refused(built, tmp_path):
    env = dict(os.environ, DMLC_ROLE="worker", DMLC_NUM_WORKER="2", DIFACTO_RANK="0", DIFACTO_DEVICE="0", DIFACTO_COMM="file",
               DIFACTO_RENDEZVOUS=str(tmp_path))
    r = _difacto(built, "task=convert", "data_format=libsvm", "data_out=%s" % (tmp_path / "o"), "data_out_format=rec", env=env)
    assert r.returncode != 0 and "task=convert" in r.stderr and "DMLC_ROLE" in r.stderr and "one process" in r.stderr, r.stderr[-2000:]


def test_device_parse_of_libsvm_is_refused(built, tmp_path):
    r = _difacto(built, "task=convert", "data_format=libsvm", "data_out=%s" % (tmp_path / "o"), "data_out_format=rec", "text_parse=device")
    assert r.returncode != 0 and "text_parse=device with data_format=libsvm" in r.stderr and "criteo" in r.stderr, r.stderr[-2000:]


def _payloads():
    rng = np.random.default_rng(3)
    body = lambda n: bytes(rng.integers(1, 200, size=n, dtype=np.uint8))   # noqa: E731  (never the magic word's bytes in a row)
    out = {}
    for k in range(4):
        out["plain_%d" % k] = body(40 + k)
        out["start_%d" % k] = MAGIC + body(36 + k)
        out["middle_%d" % k] = body(20) + MAGIC + body(16 + k)
        out["twice_in_a_row_%d" % k] = body(8) + MAGIC + MAGIC + body(12 + k)
        out["unaligned_%d" % k] = body((5, 6, 7, 9)[k]) + MAGIC + body(14 + k)
    out["last_word"] = body(24) + MAGIC
    out["last_word_then_1"] = body(24) + MAGIC + body(1)
    out["only_magic"] = MAGIC
    out["several"] = body(4) + MAGIC + body(8) + MAGIC + body(3)
    out["empty"] = b""
    out["magic_in_the_unaligned_tail"] = body(22) + MAGIC   # starts at byte 22: not at a multiple of 4
    return out


@pytest.mark.parametrize("name", sorted(_payloads()))
def test_recordio_writer(ing, name):
    from oracle import ingest as oi
    payload = _payloads()[name]
    want = oi.write_recordio([payload])
    dst = C.create_string_buffer(len(payload) + 256)
    n = ing.ingest_write_recordio(payload, len(payload), dst, len(dst))
    assert n == len(want) and dst.raw[:n] == want
    assert n % 4 == 0
    if name.startswith("unaligned") or name == "magic_in_the_unaligned_tail":
        assert want[4:8] == struct.pack("<I", len(payload)), "an unaligned magic word is not cut at"
    if name.startswith(("start", "middle", "twice", "last_word", "several", "only")):
        assert struct.unpack_from("<I", want, 4)[0] >> 29 == 1
    assert ing.ingest_write_recordio(payload, len(payload), dst, 4) == -1


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _criteo_rows(rng, n):
    rows = []
    for _ in range(n):
        ints = [b"" if rng.random() < 0.2 else b"%d" % int(rng.integers(0, 50)) for _ in range(13)]
        cats = [b"" if rng.random() < 0.15 else b"%08x" % int(rng.integers(0, 40)) for _ in range(26)]
        rows.append(b"\t".join([b"%d" % int(rng.random() < 0.3)] + ints + cats) + b"\n")
    return rows


@pytest.fixture(scope="module")
def criteo_files(tmp_path_factory):
    """3 000 generated rows; the same with one CRLF row in the middle"""
    d = tmp_path_factory.mktemp("criteo_convert")
    rows = _criteo_rows(np.random.default_rng(7), 3000)
    clean, crlf = d / "clean.txt", d / "crlf.txt"
    clean.write_bytes(b"".join(rows))
    rows[1500] = rows[1500][:-1] + b"\r\n"
    crlf.write_bytes(b"".join(rows))
    return {"clean": str(clean), "crlf": str(crlf)}


@pytest.fixture(scope="module")
def converted(built, criteo_files, tmp_path_factory):
    """both texts converted with text_parse = host and = device, chunks of 4 096 bytes: {(which, mode): (path, log)}"""
    d = tmp_path_factory.mktemp("converted")
    env = dict(os.environ, DIFACTO_CHUNK_BYTES="4096")
    out = {}
    for which in ("clean", "crlf"):
        for mode in ("host", "device"):
            path = d / ("%s_%s.rec" % (which, mode))
            r = _difacto(built, "task=convert", "data_format=criteo", "data_out=%s" % path, "data_out_format=rec", "text_parse=" + mode,
                         env=env, data=criteo_files[which])
            assert r.returncode == 0, r.stderr[-3000:]
            out[which, mode] = (str(path), r.stderr)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["clean", "crlf"])
def test_criteo_to_rec_host_and_device_parse(ing, criteo_files, converted, which):
    (host_path, host_log), (dev_path, dev_log) = converted[which, "host"], converted[which, "device"]
    host_bytes = open(host_path, "rb").read()
    assert len(host_bytes) > 100000 and host_bytes == open(dev_path, "rb").read()
    assert "text_parse" not in host_log
    m = re.search(r"text_parse=device: (\d+) of (\d+) chunks of \S+ parsed on the device, (\d+) fell back to the host parser", dev_log)
    assert m, dev_log[-3000:]
    on_device, chunks, fell_back = (int(x) for x in m.groups())
    assert on_device > 100 and on_device + fell_back == chunks
    if which == "crlf":
        assert fell_back == 1 and "WARNING" in dev_log and "were parsed on the host" in dev_log
    else:
        assert fell_back == 0 and "were parsed on the host" not in dev_log
    for log in (host_log, dev_log):
        assert "written 3000 examples in" in log and re.search(r"done. written \d+ bytes", log)
        assert len(re.findall(r"written \d+ examples in", log)) == chunks
    # one record per chunk, and the rows of the text, row for row
    assert read_all(ing, host_path, "rec") == read_all(ing, criteo_files[which], "criteo")
    assert read_all(ing, host_path, "rec")[4] == 3000


@pytest.mark.gpu
def test_training_from_the_conversion(built, criteo_files, converted):
    args = ["learner=sgd", "batch_size=300", "shuffle=0", "num_jobs_per_epoch=1", "max_num_epochs=2", "V_dim=4", "V_threshold=2", "l1=.1",
            "lr=.1", "stop_rel_objv=0", "stop_val_auc=-1e30"]
    lines = {}
    for name, data, fmt in (("text", criteo_files["clean"], "criteo"), ("rec", converted["clean", "device"][0], "rec")):
        r = _difacto(built, "data_format=" + fmt, *args, data=data)
        assert r.returncode == 0, r.stderr[-3000:]
        lines[name] = re.findall(r" - (Training: .*)$", r.stderr, re.M)
    assert len(lines["text"]) == 2 and lines["text"] == lines["rec"], "\n".join(lines["text"] + ["--"] + lines["rec"])


@pytest.mark.gpu
def test_parts(built, ing, tmp_path):
    """part_size = 1: a new part once the current one holds 1 MB (of payload, 1 000 000 bytes as the reference counts), so a
    part is below 1 MB plus one record"""
    text = b"".join(_criteo_rows(np.random.default_rng(11), 12000))
    src = tmp_path / "in.txt"
    src.write_bytes(text)
    env = dict(os.environ, DIFACTO_CHUNK_BYTES="65536")
    r = _difacto(built, "task=convert", "data_format=criteo", "data_out=%s" % (tmp_path / "out"), "data_out_format=rec", "part_size=1",
                 env=env, data=str(src))
    assert r.returncode == 0, r.stderr[-3000:]
    names = sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("out"))
    assert len(names) >= 2 and names == ["out-part_%d" % i for i in range(len(names))], names
    sizes = [int(x) for x in re.findall(r"written \d+ examples in (\d+) bytes", r.stderr)]
    largest_record = max(b - a if b > a else b for a, b in zip([0] + sizes, sizes))
    parts = [read_all(ing, tmp_path / n, "rec") for n in names]
    for n in names[:-1]:
        # (the file also holds 8 bytes of RecordIO head and up to 3 of padding per record)
        assert 1000000 <= (tmp_path / n).stat().st_size < 1000000 + largest_record + 11 * len(sizes)
    whole = read_all(ing, src, "criteo")
    assert sum(p[4] for p in parts) == 12000 == whole[4]
    assert b"".join(p[1] for p in parts) == whole[1] and b"".join(p[2] for p in parts) == whole[2]
    lens = np.concatenate([np.diff(np.frombuffer(p[0], np.uint64).astype(np.int64)) for p in parts])
    assert np.array_equal(lens, np.diff(np.frombuffer(whole[0], np.uint64).astype(np.int64)))


@pytest.mark.gpu
def test_libsvm_to_rec_to_rec_to_libsvm(built, ing, tmp_path):
    a, b, c = tmp_path / "a.rec", tmp_path / "b.rec", tmp_path / "c.libsvm"
    r = _difacto(built, "task=convert", "data_format=libsvm", "data_out=%s" % a, "data_out_format=rec")
    assert r.returncode == 0, r.stderr[-3000:]
    want = read_all(ing, DATA, "libsvm")
    assert want[4] == 100 and read_all(ing, a, "rec") == want
    vals = np.frombuffer(want[3], np.float32)
    assert not np.all(vals == 1), "rcv1 carries real values: they are kept"
    r = _difacto(built, "task=convert", "data_format=rec", "data_out=%s" % b, "data_out_format=rec", data=str(a))
    assert r.returncode == 0, r.stderr[-3000:]
    assert b.read_bytes() == a.read_bytes()
    r = _difacto(built, "task=convert", "data_format=rec", "data_out=%s" % c, "data_out_format=libsvm", data=str(a))
    assert r.returncode == 0, r.stderr[-3000:]
    got = read_all(ing, c, "libsvm")
    assert got[:3] == want[:3] and got[4] == 100
    as_text = np.array([np.float32(float("%g" % v)) for v in vals], np.float32)   # the stream's default formatting: %g, 6 digits
    assert got[3] == as_text.tobytes()
