"""One round's host plan of kad_sr_try_insert_tick (kadplan::sr_round_plan and its C entry kad_sr_plan_round in
opendht_amd/csrc/kad_searches_plan.cpp: the range checks, the bitmap's word arithmetic, the blocks, the pair lists) built
from source with AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program
(tests/cpp/sr_tick_plan_san.cpp) that feeds it exact-size arrays, and run. CPU only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_sr_round_plan_under_asan_ubsan():
    src = os.path.join(HERE, "cpp", "sr_tick_plan_san.cpp")
    plan = os.path.join(ROOT, "opendht_amd", "csrc", "kad_searches_plan.cpp")
    exe = os.path.join(HERE, "cpp", "sr_tick_plan_san")
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
                    "-o", exe, src, plan], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "PASS" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
