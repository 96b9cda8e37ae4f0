#!/usr/bin/env python
"""What task = dump costs by where its text is formatted, on one box (profiles/model_dump_ab.txt).

A synthetic model built through capi: `--entries` keys (default 1 000 000), V_dim `--v-dim` (default 64), every entry with V,
w and V normal floats (all regular: the device formats every unit), saved without optimiser state.  Then build/difacto
task=dump alternated H D H D H D (`--rounds` pairs):

  H  dump_write=host    every unit formatted by the host's fprintf from dfh_dump_entries
  D  dump_write=device  every unit formatted by the device (csrc/dfh_dumptext.hip)

Per run: entries/s and MB/s by the task's own clock (from dfh_dump_open to the renamed file: the "dumped in" seconds of its log
line; the model's load is reported beside it), the process's wall seconds, its host CPU seconds (user + sys), its peak
resident set and the largest resident set while it dumps (after the load), and whether dump_out has the bytes of the first run's.  Every run has a time limit of its own and nothing more is
started after a run that fails.  One JSON object per run and a summary on stdout.

usage: dump_ab.py [--entries 1000000] [--v-dim 64] [--rounds 3] [--unit-rows 0]"""
import argparse
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)

LINE = (r"task=dump dump_write=(\w+): (\d+) entries \((\d+) with V\) to \S+, (\d+) units / (\d+) entries formatted on the device, "
        r"(\d+) units / (\d+) entries on the host, (\d+) bytes; model loaded in ([0-9.e+-]+) s, dumped in ([0-9.e+-]+) s")
LOADED = r"loaded (\d+) entries of V_dim (\d+) from \d+ files? \((\d+) bytes in HBM\)"


def write_model(path, n, k, seed=1):
    """n entries with V through capi.Table.import_ (in pieces) and Table.save; returns the file's size"""
    from difacto_amd import capi
    rng = np.random.default_rng(seed)
    ctx = capi.Context(0)
    tb = capi.Table(ctx, n + n // 2 + 1024, V_dim=k, init_mode=capi.INIT_HASH)
    ids = rng.permutation(np.arange(1, 4 * n + 1, dtype=np.uint64))[:n] * np.uint64(2654435761)   # distinct (an odd multiplier mod 2^64)
    piece = 100000
    for a in range(0, n, piece):
        m = min(piece, n - a)
        scal = np.zeros((m, 4), np.float32)
        scal[:, 1] = rng.normal(size=m) * 0.1
        V = np.zeros((m, 2 * k), np.float32)
        V[:, :k] = rng.normal(size=(m, k)) * 0.05
        tb.import_(ids[a:a + m], scal, np.ones(m, np.int32), V if k else None)
    saved = tb.save(path, save_aux=False)
    tb.close()
    ctx.close()
    assert saved == n, (saved, n)
    return os.path.getsize(path)


def run(cmd, timeout):
    """one child under a time limit of its own: its log line's figures, wall seconds, from wait4 its own CPU seconds, and its
    resident set as /proc/<pid>/status reports it while it runs (polled; wait4's ru_maxrss starts from this process's own
    resident set at the fork and says nothing about a smaller child): the peak of the whole run (VmHWM), and the largest VmRSS
    seen after the task's "loaded ..." line, that is while it dumps"""
    import threading
    t0 = time.time()
    p = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    killer = threading.Timer(timeout, p.kill)
    killer.start()
    peak_kb, samples = [0], []

    def poll():
        while True:
            try:
                st = open("/proc/%d/status" % p.pid).read()
            except OSError:
                return
            hwm, rss = re.search(r"VmHWM:\s+(\d+) kB", st), re.search(r"VmRSS:\s+(\d+) kB", st)
            if hwm and rss:
                peak_kb[0] = max(peak_kb[0], int(hwm.group(1)))
                samples.append((time.time(), int(rss.group(1))))
            time.sleep(0.005)

    poller = threading.Thread(target=poll, daemon=True)
    poller.start()
    lines, t_loaded = [], None
    try:
        for line in p.stderr:   # to the end: the child never blocks on a full pipe
            lines.append(line)
            if t_loaded is None and re.search(LOADED, line):
                t_loaded = time.time()
        _, status, ru = os.wait4(p.pid, 0)
    finally:
        killer.cancel()
    poller.join(1.0)
    err = "".join(lines)
    dump_kb = max([r for t, r in samples if t_loaded is not None and t >= t_loaded] or [0])
    rc = os.waitstatus_to_exitcode(status)
    p.returncode = rc   # reaped here, not by Popen
    m, l = re.search(LINE, err), re.search(LOADED, err)
    out = dict(rc=rc, wall_s=time.time() - t0, cpu_s=ru.ru_utime + ru.ru_stime, peak_rss_mb=peak_kb[0] / 1024.0, dump_phase_rss_mb=dump_kb / 1024.0,
               tail=err[-600:] if rc or not m else "")
    if m:
        out.update(write=m.group(1), entries=int(m.group(2)), with_V=int(m.group(3)), dev_units=int(m.group(4)), dev_entries=int(m.group(5)),
                   host_units=int(m.group(6)), host_entries=int(m.group(7)), bytes=int(m.group(8)), load_s=float(m.group(9)),
                   dump_s=float(m.group(10)))
        out.update(entries_per_s=out["entries"] / out["dump_s"], mb_per_s=out["bytes"] / 1e6 / out["dump_s"])
    if l:
        out.update(table_bytes=int(l.group(3)))
    return out


def digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest(), os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1000000)
    ap.add_argument("--v-dim", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--unit-rows", type=int, default=0, help="dump_unit_rows (0: the default)")
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="dump_ab_")
    try:
        measure(a, d)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def measure(a, d):
    model, out = os.path.join(d, "model"), os.path.join(d, "dump.txt")
    t0 = time.time()
    size = write_model(model, a.entries, a.v_dim)
    print(json.dumps(dict(model=True, entries=a.entries, V_dim=a.v_dim, model_file_mb=size / 1e6, seconds=time.time() - t0)), flush=True)
    exe = os.path.join(R, "build", "difacto")
    unit = ["dump_unit_rows=%d" % a.unit_rows] if a.unit_rows else []
    runs, want = {"host": [], "device": []}, None
    for rnd in range(a.rounds):
        for how in ("host", "device"):
            o = run([exe, "task=dump", "model_in=" + model, "dump_out=" + out, "dump_write=" + how] + unit, a.timeout)
            o.update(variant=how, round=rnd)
            if o["rc"] == 0:
                got = digest(out)
                want = want or got
                o.update(same_bytes_as_first=got == want)
                os.remove(out)
            print(json.dumps(o), flush=True)
            if o["rc"] != 0 or "dump_s" not in o:
                sys.exit("dump_write=%s failed (exit %d)" % (how, o["rc"]))   # nothing more is started after a failed run
            runs[how].append(o)
    summary = dict(summary=True, entries=a.entries, V_dim=a.v_dim, dump_out_bytes=want[1])
    for how, rs in runs.items():
        summary[how] = {k: sorted(round(o[k], 3) for o in rs) for k in ("entries_per_s", "mb_per_s", "dump_s", "load_s", "wall_s", "cpu_s", "peak_rss_mb", "dump_phase_rss_mb")}
        summary[how]["same_bytes_as_first"] = all(o["same_bytes_as_first"] for o in rs)
    summary["device_not_slower_in_every_pair"] = all(dv["dump_s"] <= h["dump_s"] for h, dv in zip(runs["host"], runs["device"]))
    summary["table_bytes"] = runs["device"][0].get("table_bytes")
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
