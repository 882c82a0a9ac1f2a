"""The kernels of opendht_amd/csrc/kad_maint.h compiled for gfx950 with
-Rpass-analysis=kernel-resource-usage: each of the six exists once and spills nothing to scratch. The engine is one
translation unit, so the same compile is run on a copy of kad_engine.hip without the kad_maint.h include: every other
kernel's resource lines must be identical in both, i.e. the new header changes no kernel that was there before it. A
cross-compile of the device code; needs no GPU."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "opendht_amd", "csrc")
NEW = ("12touch_kernel", "18btime_patch_kernel", "19btime_gather_kernel", "18maint_count_kernel", "17maint_scan_kernel",
       "18maint_write_kernel")


def _resources(src):
    r = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "-fPIC", "--cuda-device-only", "-I" + CSRC, "-Rpass-analysis=kernel-resource-usage", "-c", src,
                        "-o", os.devnull], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    seen, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            seen[name][m.group(1).strip()] = int(m.group(2))
    return seen


def test_maint_kernels_and_untouched_neighbours(tmp_path):
    src = os.path.join(CSRC, "kad_engine.hip")
    text = open(src).read()
    assert text.count('#include "kad_maint.h"\n') == 1
    without = tmp_path / "kad_engine_without_maint.hip"
    without.write_text(text.replace('#include "kad_maint.h"\n', ""))
    with ThreadPoolExecutor(2) as ex:
        a, b = ex.map(_resources, (src, str(without)))
    is_new = lambda k: any(n in k for n in NEW)
    for n in NEW:
        hits = [k for k in a if n in k]
        assert len(hits) == 1, (n, hits)
        v = a[hits[0]]
        print(hits[0], v)
        assert v["ScratchSize"] == 0, (hits[0], v)
    assert not any(is_new(k) for k in b)
    old = {k: v for k, v in a.items() if not is_new(k)}
    assert len(old) > 300 and old.keys() == b.keys()
    diff = {k: (old[k], b[k]) for k in old if old[k] != b[k]}
    assert not diff, diff
