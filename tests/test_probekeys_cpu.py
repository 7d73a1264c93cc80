"""The host arithmetic of the key-only probe side of plain count joins (hashmergejoin_amd/csrc/hmj_probekeys.h), plain and
under sanitizers.

tests/cpp/test_probekeys.cc is a stand-alone program against that header alone: the pilot's sample rule (indices in range
and strictly increasing, for probe sides below the sample count and for sizes that are no multiple of it), the decision
function over memo states and switches (attempt, pilot, skip), and the slab capacity of key rows.  It is built twice with
g++, plain and with AddressSanitizer + UBSan, and both binaries must pass every case without a sanitizer report.  Nothing
here loads libhmj_hip.so, uses HIP or touches a GPU; every file goes to tmp_path."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "test_probekeys.cc")
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
    assert "all probe-keys cases passed" in txt, "%s:\n%s" % (name, txt[-20000:])
    for rep in REPORTS:
        assert rep not in txt, "%s reported %r:\n%s" % (name, rep, txt[-20000:])


def test_probekeys_plain(tmp_path):
    _build_and_run(_gxx(), [], "test_probekeys", tmp_path)


def test_probekeys_under_sanitizers(tmp_path):
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
    _build_and_run(gxx, ASAN, "test_probekeys_asan", tmp_path)
