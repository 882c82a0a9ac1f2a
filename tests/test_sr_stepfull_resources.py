"""step_full_kernel compiled for gfx950 with -Rpass-analysis=kernel-resource-usage: both forms (16-byte
flag units, and the byte path) spill nothing to scratch and use no LDS, and the kernels §7.19 names (step_kernel,
step_expire_kernel, entries_kernel, insert_kernel, refill_kernel, try_insert_kernel, tick_verdict_kernel) still spill
nothing. A cross-compile of opendht_amd/csrc/kad_searches.hip's device code; needs no GPU."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_step_full_kernels_use_no_scratch():
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
    new = ("16step_full_kernelILb1E", "16step_full_kernelILb0E")
    kinds = {k: 0 for k in new + ("11step_kernelILb1E", "11step_kernelILb0E", "18step_expire_kernel", "14entries_kernel",
                                  "13insert_kernel", "13refill_kernel", "try_insert_kernelILb1E", "try_insert_kernelILb0E",
                                  "tick_verdict_kernelILb1E", "tick_verdict_kernelILb0E")}
    for k, v in seen.items():
        for kind in kinds:
            if kind in k:
                kinds[kind] += 1
                assert v["ScratchSize"] == 0, (k, v)
                print(k, v)
                if kind in new:
                    assert v["LDS Size"] == 0, (k, v)
    assert all(n == 1 for n in kinds.values()), (kinds, list(seen))
