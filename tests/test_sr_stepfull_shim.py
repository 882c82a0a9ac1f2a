"""Compiles and runs tests/cpp/test_sr_stepfull_shim.cpp: include/kadgpu.hpp's SearchesMirror::markDue / stepBatchFull and
DhtMirror::markSearchDue / stepSearchesFull over OpenDHT-shaped test doubles that keep getStatus, listenStatus, acked and
probe_query as fields and run their own three send loops of searchStep entry by entry: a snapshot, the step bits sent with
markEntries and the due bits with markDue, a step in verdict mode, two applied steps with replies, acks and expired
listens in between, the device export compared with the host's lists after each. Compiled here with the flags of
tests/test_refill_shim.py."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build():
    src = os.path.join(HERE, "cpp", "test_sr_stepfull_shim.cpp")
    exe = os.path.join(HERE, "cpp", "test_sr_stepfull_shim")
    deps = [src, os.path.join(ROOT, "include", "kadgpu.hpp"), os.path.join(ROOT, "include", "kadgpu.h"),
            os.path.join(ROOT, "opendht_amd", "libkadgpu.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        "-o", exe, src, "-L" + os.path.join(ROOT, "opendht_amd"), "-lkadgpu",
                        "-L" + os.path.join(ROOT, "oracle"), "-loracle", "-Wl,-rpath,$ORIGIN/../../opendht_amd",
                        "-Wl,-rpath,$ORIGIN/../../oracle"], check=True)
    return exe


def test_sr_stepfull_shim_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_sr_stepfull_shim_parity():
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout
