"""rec_decode = device on the command line: learner = sgd's device feed and task = convert read a .rec file whose records the
device decodes (host/device_rec_decode.h, csrc/dfh_lz4dec.hip).

No GPU: the key's values and the combinations that are refused before the device is touched, in the cases and wording of
text_parse = device.  GPU: training and conversion give the same results wherever the records are inflated, a record that carries
values falls back to the host decoder and is counted, and the job's line says how many records went which way."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
REC_MAGIC = 0xced7230a


@pytest.fixture(scope="module")
def built():
    from difacto_amd import build
    build.build_hip()
    build.build_host()
    return os.path.join(ROOT, "build")


def _difacto(built, *args, env=None, data=DATA, timeout=300):
    return subprocess.run([os.path.join(built, "difacto"), "data_in=" + data] + list(args), capture_output=True, text=True, timeout=timeout,
                          cwd=ROOT, env=env)


# ---------------------------------------------------------------------------------------------------------------------
# the key's values and the combinations that are refused (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
REQUIRED = ["batch_size=25", "V_dim=4"]


def test_unknown_value_is_fatal(built):
    r = _difacto(built, *REQUIRED, "rec_decode=disk", "data_format=rec")
    assert r.returncode != 0 and "rec_decode=disk" in r.stderr and "host" in r.stderr and "device" in r.stderr, r.stderr[-2000:]


@pytest.mark.parametrize("fmt", ["libsvm", "criteo", "adfea"])
def test_other_formats_are_refused(built, fmt):
    r = _difacto(built, *REQUIRED, "rec_decode=device", "data_format=" + fmt, "shuffle=2")
    assert r.returncode != 0 and "rec_decode=device with data_format=" + fmt in r.stderr and "rec files only" in r.stderr, r.stderr[-2000:]


def test_literal_path_is_refused(built):
    r = _difacto(built, *REQUIRED, "rec_decode=device", "data_format=rec", "shuffle=2", "device_path=literal")
    assert r.returncode != 0 and "rec_decode=device with device_path=literal" in r.stderr, r.stderr[-2000:]


def test_a_rank_is_refused(built, tmp_path):
    env = dict(os.environ, DMLC_ROLE="worker", DMLC_NUM_WORKER="2", DIFACTO_RANK="0", DIFACTO_DEVICE="0", DIFACTO_COMM="file",
               DIFACTO_RENDEZVOUS=str(tmp_path))
    r = _difacto(built, *REQUIRED, "rec_decode=device", "data_format=rec", "shuffle=2", env=env)
    assert r.returncode != 0 and "rec_decode=device with a sharded store" in r.stderr, r.stderr[-2000:]


@pytest.mark.parametrize("learner", ["lbfgs", "bcd"])
def test_other_learners_are_refused(built, learner):
    r = _difacto(built, *REQUIRED, "rec_decode=device", "data_format=rec", "learner=" + learner)
    assert r.returncode != 0 and "rec_decode=device with learner=" + learner in r.stderr and "learner=sgd" in r.stderr, r.stderr[-2000:]


def test_no_shuffle_buffer_is_refused(built):
    r = _difacto(built, *REQUIRED, "rec_decode=device", "data_format=rec", "shuffle=0")
    assert r.returncode != 0 and "rec_decode=device without a shuffle buffer" in r.stderr, r.stderr[-2000:]


def test_convert_refuses_other_formats_and_values(built, tmp_path):
    out = "data_out=%s" % (tmp_path / "o.rec")
    r = _difacto(built, "task=convert", "data_format=criteo", "data_out_format=rec", out, "rec_decode=device")
    assert r.returncode != 0 and "rec_decode=device with data_format=criteo" in r.stderr, r.stderr[-2000:]
    r = _difacto(built, "task=convert", "data_format=rec", "data_out_format=rec", out, "rec_decode=gpu")
    assert r.returncode != 0 and "rec_decode=gpu is not one of host (the default) and device" in r.stderr, r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------------------------------
# training and conversion (GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _read_recordio(blob):
    """the records of a .rec file (dmlc RecordIO: magic, cflag << 29 | length, payload padded to 4 bytes; a record that holds the
    magic word at an aligned position is stored in parts, cflag 1 .. 3, the word between them left out)"""
    recs, at, parts = [], 0, None
    magic = struct.pack("<I", REC_MAGIC)
    while at < len(blob):
        assert blob[at:at + 4] == magic
        h = struct.unpack_from("<I", blob, at + 4)[0]
        flag, n = h >> 29, h & ((1 << 29) - 1)
        payload = blob[at + 8:at + 8 + n]
        at += 8 + (n + 3) // 4 * 4
        if flag == 0:
            recs.append(payload)
        elif flag == 1:
            parts = [payload]
        else:
            parts.append(payload)
            if flag == 3:
                recs.append(magic.join(parts))
                parts = None
    return recs


@pytest.fixture(scope="module")
def rec_files(built, tmp_path_factory):
    """3 000 generated criteo rows converted to .rec by task = convert in records of about 50 KB of text; the same file with one
    record spliced in that carries values (not all 1): it is not regular and the host decoder takes it"""
    d = tmp_path_factory.mktemp("rec_cli")
    rng = np.random.default_rng(7)
    rows = []
    for _ in range(3000):
        ints = [b"" if rng.random() < 0.2 else b"%d" % int(rng.integers(0, 50)) for _ in range(13)]
        cats = [b"" if rng.random() < 0.15 else b"%08x" % int(rng.integers(0, 40)) for _ in range(26)]
        rows.append(b"\t".join([b"%d" % int(rng.random() < 0.3)] + ints + cats) + b"\n")
    text = d / "clean.txt"
    text.write_bytes(b"".join(rows))
    clean = d / "clean.rec"
    r = _difacto(built, "task=convert", "data_format=criteo", "data_out_format=rec", "data_out=%s" % clean, "chunk_size=0.05", data=str(text))
    assert r.returncode == 0, r.stderr[-3000:]
    recs = _read_recordio(clean.read_bytes())
    assert len(recs) >= 4
    from difacto_amd import capi
    from oracle import ingest as oi
    ctx = capi.Context(0)
    enc = capi.CrbEncoder(ctx)
    off = np.arange(0, 39 * 61, 39, dtype=np.uint64)
    idx = (rng.integers(0, 40, size=int(off[-1]), dtype=np.uint64) << np.uint64(12)) | (np.arange(int(off[-1]), dtype=np.uint64) % np.uint64(39))
    val = np.ones(len(idx), np.float32)
    val[::7] = 0.5
    valued = enc.encode_host(off, (rng.random(60) < 0.3).astype(np.float32), idx, val)
    enc.close()
    ctx.close()
    mixed = d / "mixed.rec"
    mixed.write_bytes(oi.write_recordio(recs[:2] + [valued] + recs[2:]))
    return {"clean": str(clean), "mixed": str(mixed), "records": {"clean": len(recs), "mixed": len(recs) + 1}}


def _model_records(blob):
    """model_out as (header, records sorted by key), every byte of it.  The file lists the table's rows in the order the keys
    were first inserted, which the insert's atomics decide anew in every run (two runs with rec_decode=host differ in it too;
    tests/test_text_parse.py and tests/test_sgd_data_cache.py sort by key for the same reason): the comparison is of all the
    bytes, the records in key order.  Layout (dfh_table_save, with optimiser state): "DFHM", version, V_dim, aux = 1, count;
    per entry key u64, w, {fea_cnt, sqrt_g, z}, has_V i32, then V and its accumulators (2 x V_dim floats) iff has_V"""
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


CLI_CONFIGS = {"plain": [], "data_cache": ["data_cache=hbm"]}


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["clean", "mixed"])
@pytest.mark.parametrize("config", sorted(CLI_CONFIGS))
def test_training_does_not_depend_on_where_the_records_are_decoded(built, tmp_path, rec_files, config, which):
    """2 epochs, shuffle = 2: the Training lines string for string, model_out byte for byte (its records in key order); 0
    fallbacks on the clean file, exactly 1 per pass over the file on the one with the spliced record"""
    runs = {}
    for mode in ("host", "device"):
        model = tmp_path / ("model_" + mode)
        r = _difacto(built, "data_format=rec", "batch_size=300", "shuffle=2", "V_dim=4", "max_num_epochs=2", "V_threshold=2", "l1=.1",
                     "lr=.1", "stop_rel_objv=0", "stop_val_auc=-1e30", "model_out=%s" % model, "rec_decode=" + mode, *CLI_CONFIGS[config],
                     data=rec_files[which])
        assert r.returncode == 0, r.stderr[-3000:]
        runs[mode] = (re.findall(r" - (Training: .*)$", r.stderr, re.M), model.read_bytes(), r.stderr)
    (lines_h, model_h, log_h), (lines_d, model_d, log_d) = runs["host"], runs["device"]
    assert len(lines_h) == 2 and lines_h == lines_d, "\n".join(lines_h + ["--"] + lines_d)
    assert len(model_h) > 1000 and len(model_h) == len(model_d) and _model_records(model_h) == _model_records(model_d)
    assert "rec_decode" not in log_h
    counts = re.findall(r"rec_decode=device: (\d+) of (\d+) records of \S+ decoded on the device, (\d+) fell back to the host decoder", log_d)
    assert counts, log_d[-3000:]
    on_device, records, fell_back = (sum(int(c[i]) for c in counts) for i in range(3))
    passes = 1 if config == "data_cache" else 2   # (a cached part is not read again)
    assert records == passes * rec_files["records"][which] and on_device + fell_back == records
    if which == "mixed":
        assert fell_back == passes and "WARNING" in log_d and "were inflated on the host" in log_d, log_d[-3000:]
    else:
        assert fell_back == 0 and "were inflated on the host" not in log_d


@pytest.mark.gpu
@pytest.mark.parametrize("order", [["shuffle_rows=1", "shuffle_seed=1"], []])
def test_convert_does_not_depend_on_where_the_records_are_decoded(built, tmp_path, rec_files, order):
    """task = convert of a .rec into a .rec: shuffled through the row store, and record by record"""
    outs = {}
    for mode in ("host", "device"):
        out = tmp_path / ("out_%s.rec" % mode)
        r = _difacto(built, "task=convert", "data_format=rec", "data_out_format=rec", "data_out=%s" % out, "rec_decode=" + mode, *order,
                     data=rec_files["clean"])
        assert r.returncode == 0, r.stderr[-3000:]
        outs[mode] = (out.read_bytes(), r.stderr)
    assert len(outs["host"][0]) > 10000 and outs["host"][0] == outs["device"][0]
    assert "rec_decode" not in outs["host"][1]
    m = re.search(r"rec_decode=device: (\d+) of (\d+) records of \S+ decoded on the device, 0 fell back to the host decoder", outs["device"][1])
    assert m and int(m.group(1)) == int(m.group(2)) == rec_files["records"]["clean"], outs["device"][1][-3000:]
    if not order:
        assert outs["host"][0] == open(rec_files["clean"], "rb").read()   # (the encoder gives the same bytes for the same rows)
