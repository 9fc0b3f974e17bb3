"""CPU: the create-time choices of shim/tune.hpp -- which CSR-vector form, packed planes or not, which blocked form, which depth of the rows
kernel -- are pure functions of the measured times.  tests/c/tune_rules_check.cpp compiles that header alone (no HIP), under ASan + UBSan,
and runs every rule and the form table against the expressions they replaced, over every combination of a set of times."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spmv_amd", "csrc")


def test_rules_and_form_table_match_the_expressions_they_replaced(tmp_path):
    exe = str(tmp_path / "tune_rules_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{CSRC}", os.path.join(ROOT, "tests", "c", "tune_rules_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr, r.stdout + r.stderr
    m = re.search(r"tune rules: (\d+) cases, 0 failures", r.stdout)
    # 2 x 6^5 vector + 6^5 packed + 2 x 6^2 blocked and rows + 16 codes x 2 value sizes x (4 + 3) table
    assert m and int(m.group(1)) == 3 * 6 ** 5 + 2 * 6 ** 2 + 16 * 2 * 7, r.stdout
