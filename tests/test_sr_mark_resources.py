"""The three kernels of kad_sr_mark_nodes compiled for gfx950 with
-Rpass-analysis=kernel-resource-usage: none of them may spill to scratch, and the scan kernel's LDS form holds the 4096
batch keys and their prefix directory. A cross-compile of opendht_amd/csrc/kad_searches.hip's device code; needs no
GPU."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_mark_kernels_use_no_scratch():
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
    marks = {k: v for k, v in seen.items() if "mark_" in k}
    kinds = {"mark_scan_kernelILb1E": 0, "mark_scan_kernelILb0E": 0, "mark_pairs_kernel": 0, "mark_fix_kernel": 0}
    for k, v in marks.items():
        assert v["ScratchSize"] == 0, (k, v)
        for kind in kinds:
            kinds[kind] += kind in k
        if "mark_scan_kernelILb1E" in k:  # 4096 keys of 8 bytes, 2^11 + 2 directory bounds of 2 bytes
            assert 4096 * 8 + 2 * ((1 << 11) + 1) <= v["LDS Size"] <= 40 * 1024, v
        else:
            assert v["LDS Size"] == 0, (k, v)
    assert all(n == 1 for n in kinds.values()), (kinds, list(marks))
    # the kernels beside them keep what DESIGN.md records
    for k, v in seen.items():
        if "refill_kernel" in k or "insert_kernel" in k:
            assert v["ScratchSize"] == 0, (k, v)
