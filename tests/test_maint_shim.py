"""Compiles and runs tests/cpp/test_maint_shim.cpp: include/kadgpu.hpp's RoutingTableMirror::bucketMaintenance,
onReportedAddrBatch, onReportedAddr, resetBucketTimes, the upload of Bucket::time by snapshot, flush after splits and
the DhtMirror forwarders over OpenDHT-shaped test doubles and std::mt19937 at fixed seeds: the pick and the generator's
state against the reference's loop restated on the doubles. Compiled here with the flags of tests/cpp/Makefile's
test_shim rule."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _build():
    src = os.path.join(HERE, "cpp", "test_maint_shim.cpp")
    exe = os.path.join(HERE, "cpp", "test_maint_shim")
    deps = [src, os.path.join(ROOT, "include", "kadgpu.hpp"), os.path.join(ROOT, "include", "kadgpu.h"),
            os.path.join(ROOT, "opendht_amd", "libkadgpu.so")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run([os.environ.get("CXX", "g++"), "-O2", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        "-o", exe, src, "-L" + os.path.join(ROOT, "opendht_amd"), "-lkadgpu",
                        "-Wl,-rpath,$ORIGIN/../../opendht_amd"], check=True)
    return exe


def test_maint_shim_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_maint_shim_parity():
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout
