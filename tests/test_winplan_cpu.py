"""The planning of hmj_window_device (hashmergejoin_amd/csrc/hmj_winplan.h) on the host, plain and under sanitizers.

tests/cpp/test_winplan.cc is a stand-alone program against that header alone: consistent grids and carry levels for every
boundary size, what every function writes, and a cut of the functions into launches that covers every function once.  It is
built twice with g++, plain and with AddressSanitizer + UBSan, and both binaries must pass every case without a sanitizer
report.  The program prints the kernels' constants P (positions per wave), G (positions per workgroup) and T (aggregates
per carry tile): they must be the literals tests/test_window_gpu.py sizes its cases with, and 2^22 + 77 rows must reach the
carry's top level.  Nothing here loads libhmj_hip.so, uses HIP or touches a GPU; every file goes to tmp_path."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "test_winplan.cc")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:")
TRIVIAL = "int main() { return 0; }\n"


def _gxx():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    return gxx


def _compile(gxx, flags, src, exe):
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", *flags, src, "-o", exe]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)


def _build_and_run(gxx, flags, name, tmp_path):
    exe = str(tmp_path / name)
    out = _compile(gxx, flags, SOURCE, exe)
    assert out.returncode == 0, "%s build failed:\n%s" % (name, out.stdout.decode(errors="replace"))
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=str(tmp_path))
    txt = run.stdout.decode(errors="replace")
    assert run.returncode == 0, "%s exited with %d:\n%s" % (name, run.returncode, txt[-20000:])
    assert "all window plan cases passed" in txt, "%s:\n%s" % (name, txt[-20000:])
    for rep in REPORTS:
        assert rep not in txt, "%s reported %r:\n%s" % (name, rep, txt[-20000:])
    return txt


def test_winplan_plain_and_its_constants_are_the_gpu_tests_literals(tmp_path):
    txt = _build_and_run(_gxx(), [], "test_winplan", tmp_path)
    printed = {k: int(v) for k, v in re.findall(r"^(P|G|T|top|levels\(2\^22\+77\)) (\d+)$", txt, flags=re.M)}
    src = open(os.path.join(ROOT, "tests", "test_window_gpu.py")).read()
    literals = {k: int(v) for k, v in re.findall(r"^(P|G|T) = (\d+)\b", src, flags=re.M)}
    assert literals == {"P": 512, "G": 2048, "T": 2048}
    assert {k: printed[k] for k in "PGT"} == literals
    assert printed["levels(2^22+77)"] == printed["top"] == 2  # test_window_gpu.py's largest case crosses carry tiles


def test_winplan_under_sanitizers(tmp_path):
    gxx = _gxx()
    # a sanitizer whose trivial program does not build or run here (no runtime library, a kernel it cannot map) is skipped
    src = tmp_path / "trivial.cc"
    src.write_text(TRIVIAL)
    exe = str(tmp_path / "trivial_asan")
    ok = _compile(gxx, ASAN, str(src), exe).returncode == 0
    if ok:
        try:
            ok = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60).returncode == 0
        except subprocess.TimeoutExpired:
            ok = False
    if not ok:
        pytest.skip("a trivial program built with g++ -fsanitize=address,undefined does not run here")
    _build_and_run(gxx, ASAN, "test_winplan_asan", tmp_path)
