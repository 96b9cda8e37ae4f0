"""The line arithmetic of explain_out and recommend_out on the host (no GPU): csrc/dfh_listtext_fmt.h is plain C++ over the two
older _fmt.h headers, so tools/list_fmt_check.cc compiles the very functions the device formatter calls, with g++
-fsanitize=address,undefined, and compares whole lines with the learner's snprintf calls: every list length 0 .. K for K in
{1, 10, 32}, ids and items of every digit count, designed floats, the longest lines in blocks of exactly the documented
maximum, 20 000 random lines per kind; a float outside the regular range must be counted."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lines_equal_snprintf(tmp_path):
    exe = str(tmp_path / "list_fmt_check")
    cc = ["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-std=c++14", "-Wno-unknown-pragmas",
          "-I" + os.path.join(ROOT, "difacto_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tools", "list_fmt_check.cc")]
    r = subprocess.run(cc, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    m = re.search(r"ok: (\d+) lines, (\d+) entries, 20000 random lines per kind", r.stdout)
    assert m and int(m.group(1)) > 40000 and int(m.group(2)) > 200000, out[-2000:]
