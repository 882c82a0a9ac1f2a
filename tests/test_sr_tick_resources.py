"""The kernels of kad_sr_try_insert_tick compiled for gfx950 with
-Rpass-analysis=kernel-resource-usage: the verdict kernel in both forms and the gather kernel spill nothing to scratch,
the verdict kernel's LDS form holds the 4096 search keys, and the kernels beside them (insert_kernel, which the tick
runs unmodified, refill_kernel and try_insert_kernel) still spill nothing. A cross-compile of
opendht_amd/csrc/kad_searches.hip's device code; needs no GPU."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_tick_kernels_use_no_scratch():
    src = os.path.join(ROOT, "opendht_amd", "csrc", "kad_searches.hip")
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        os.devnull], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    seen = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            seen[name][m.group(1).strip()] = int(m.group(2))
    kinds = {"tick_verdict_kernelILb1E": 0, "tick_verdict_kernelILb0E": 0, "tick_gather_kernel": 0,
             "13insert_kernel": 0, "13refill_kernel": 0, "try_insert_kernelILb1E": 0, "try_insert_kernelILb0E": 0}
    for k, v in seen.items():
        for kind in kinds:
            if kind in k:
                kinds[kind] += 1
                assert v["ScratchSize"] == 0, (k, v)
                print(k, v)
                if kind in ("tick_verdict_kernelILb1E", "try_insert_kernelILb1E"):
                    assert 4096 * 8 <= v["LDS Size"] <= 33 * 1024, (k, v)
                else:
                    assert v["LDS Size"] == 0, (k, v)
    assert all(n == 1 for n in kinds.values()), (kinds, list(seen))
