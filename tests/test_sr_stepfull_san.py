"""The host parts of kad_sr_step_full and kad_sr_mark_due (kad_search_step_full and kad_search_step_full_batch over
kadstep::decide_full of opendht_amd/csrc/kad_step.h, the function the kernel calls; kadplan::sr_step_full_check and
kadplan::sr_due_plan in opendht_amd/csrc/kad_searches_plan.cpp) built from source with AddressSanitizer and
UndefinedBehaviorSanitizer into a stand-alone program (tests/cpp/sr_stepfull_san.cpp) that feeds them exact-size arrays,
and run as a process. CPU only."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_step_full_host_parts_under_asan_ubsan():
    src = os.path.join(HERE, "cpp", "sr_stepfull_san.cpp")
    plan = os.path.join(ROOT, "opendht_amd", "csrc", "kad_searches_plan.cpp")
    exe = os.path.join(HERE, "cpp", "sr_stepfull_san")
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"),
                    "-o", exe, src, plan], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "PASS" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
