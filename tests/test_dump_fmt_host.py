"""The line arithmetic of task = dump on the host (no GPU): csrc/dfh_dumptext_fmt.h (the id's digits, a field, where things go
in a line) over csrc/dfh_predtext_fmt.h (the floats) are plain C++, so tools/dump_fmt_check.cc compiles the very functions the
device formatter calls, with g++ -fsanitize=address,undefined, and compares whole lines "<id>\\t<w>[\\t<V_j>]\\n" with snprintf:
ids of every digit count 1 .. 20 (1, 9, 10, 99, 100, ..., 10^19, 2^64 - 2), V_dim 0, 1 and 64, designed values (+-0, ties,
both ends of the regular range) and 10^5 random bit patterns; a value outside the regular range must be reported, not
formatted.  Each line is assembled in a heap block of exactly the documented maximum, 20 + 16 (1 + V_dim) + 1 bytes."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dump_fmt") / "dump_fmt_check")
    cc = ["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g", "-std=c++14", "-Wno-unknown-pragmas",
          "-I" + os.path.join(ROOT, "difacto_amd", "csrc"), "-o", out, os.path.join(ROOT, "tools", "dump_fmt_check.cc")]
    r = subprocess.run(cc, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_lines_equal_snprintf(exe):
    r = subprocess.run([exe, "100000"], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    m = re.search(r"ok: (\d+) lines, (\d+) values, (\d+) irregular values reported, 100000 random bit patterns", r.stdout)
    assert m, out[-2000:]
    lines, values, irregular = (int(x) for x in m.groups())
    # 96 of the 256 biased exponents are regular: about 3/8 of the patterns fill lines (thrice: V_dim 0, 1, 64), the rest are reported
    assert 55000 < irregular < 70000 and values > 3 * (100000 - irregular) and lines > 2 * (100000 - irregular)


def test_the_header_is_plain_cpp():
    """no HIP in the header: a host program includes nothing but it (and the float formatter it builds on)"""
    src = open(os.path.join(ROOT, "difacto_amd", "csrc", "dfh_dumptext_fmt.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', src) == ["dfh_predtext_fmt.h"]
    assert "hip/" not in src and "__global__" not in src and "threadIdx" not in src
