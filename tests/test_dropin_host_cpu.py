"""The C++ drop-in operator (include/hashmergejoin_hip.hpp) on the host, under sanitizers.

tests/cpp/test_dropin_host.cc is linked against tests/cpp/hmj_abi_stub.cc, a host implementation of the C ABI calls the
header makes, and built twice with g++: with AddressSanitizer + UBSan and with ThreadSanitizer.  Both binaries must pass
every case without a sanitizer report.  Nothing here loads libhmj_hip.so or touches a GPU; every file goes to tmp_path."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SOURCES = [os.path.join(CPP, "test_dropin_host.cc"), os.path.join(CPP, "hmj_abi_stub.cc")]
SANITIZERS = {
    "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
    "tsan": ["-fsanitize=thread"],
}
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:", "WARNING: ThreadSanitizer")
TRIVIAL = "#include <thread>\nint main() { std::thread t([] {}); t.join(); return 0; }\n"


def _gxx():
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    return gxx


def _compile(gxx, flags, srcs, exe):
    cmd = [gxx, "-std=c++11", "-g", "-O1", *flags, "-I" + os.path.join(ROOT, "include"), *srcs, "-o", exe, "-pthread"]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)


def _sanitizer_runs(gxx, name, tmp_path):
    # a sanitizer whose trivial program does not build or run here (no runtime library, a kernel it cannot map) is skipped
    src = tmp_path / "trivial.cc"
    src.write_text(TRIVIAL)
    exe = str(tmp_path / ("trivial_" + name))
    if _compile(gxx, SANITIZERS[name], [str(src)], exe).returncode != 0:
        return False
    try:
        return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60).returncode == 0
    except subprocess.TimeoutExpired:
        return False


def test_dropin_host_under_sanitizers(tmp_path):
    gxx = _gxx()
    for name in SANITIZERS:
        if not _sanitizer_runs(gxx, name, tmp_path):
            pytest.skip("a trivial program built with g++ -fsanitize for %s does not run here" % name)

    def build_and_run(name):  # the two builds and runs overlap: one g++ or one test process per sanitizer
        exe = str(tmp_path / ("test_dropin_host_" + name))
        out = _compile(gxx, SANITIZERS[name], SOURCES, exe)
        assert out.returncode == 0, "%s build failed:\n%s" % (name, out.stdout.decode(errors="replace"))
        return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, cwd=str(tmp_path))

    with ThreadPoolExecutor(len(SANITIZERS)) as pool:
        runs = {name: pool.submit(build_and_run, name) for name in SANITIZERS}
        for name, r in runs.items():
            out = r.result()
            txt = out.stdout.decode(errors="replace")
            assert out.returncode == 0, "%s run exited with %d:\n%s" % (name, out.returncode, txt[-20000:])
            assert "all host drop-in cases passed" in txt, "%s run:\n%s" % (name, txt[-20000:])
            for rep in REPORTS:
                assert rep not in txt, "%s run reported %r:\n%s" % (name, rep, txt[-20000:])
