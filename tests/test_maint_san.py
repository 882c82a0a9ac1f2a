"""The host twin of kad_table_maintenance (kad_maint_scan_host, opendht_amd/csrc/kad_maint_host.cpp) and
kadmaint::kind_of (kad_maint_kind.h, the function the kernels call) built from source with AddressSanitizer and
UndefinedBehaviorSanitizer into a stand-alone program (tests/cpp/maint_san.cpp) that feeds them exact-size arrays for
every B from 0 to 70 and compares with loops written out in C++, and run as a process. CPU only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_maint_host_twin_under_asan_ubsan():
    src = os.path.join(HERE, "cpp", "maint_san.cpp")
    twin = os.path.join(ROOT, "opendht_amd", "csrc", "kad_maint_host.cpp")
    exe = os.path.join(HERE, "cpp", "maint_san")
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
                    "-o", exe, src, twin], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "PASS" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
