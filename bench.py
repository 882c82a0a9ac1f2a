"""Headline bench: k=8 closest-node queries/sec at a 100M-node table (1/8 per GPU) + % HBM roofline.

Workload (BASELINE.json config 3, per GPU): rank r holds shard r of the 100M-node U(24)
routing table (2^21 owned buckets, ~12.5M nodes, plus the exact halo from its neighbours) in
HBM and answers batches of 1,048,576 RoutingTable::findClosestNodes(target, now, 8) queries
whose targets it owns. One step = one batched kernel launch over one batch. Every timed step
reads a DIFFERENT batch of targets and writes a different output buffer (all resident in HBM
before the timed region), so no step re-reads the previous step's targets or rows out of the
256 MiB Infinity Cache. Weak scaling: per-GPU work is fixed as N grows; at N=8 the shards cover
the whole 100M-node table and a step answers 8M queries. No data-path collective (owner
routing).

A plain run does only that: set up, warm up, time the K steps, print the line. More than 128
steps rotate over 128 batches (27 times the Infinity Cache), and more than 2048 go out as replays
of one HIP graph of 2048 launches. --dump-outputs DIR writes the last timed step's rows and counts
as DIR/idx.npy and DIR/cnt.npy (dump_outputs).

With --full the same line carries the check of the last step's rows against the CPU restatement
(`verified`), the north-star variant as `allgather` (the 100M-node
table split over the N GPUs without halo, 1M global queries per step replicated on every rank,
RCCL all-gather of rows and parts + device merge), the status-refresh cost (`refresh`), the other
passes of DESIGN.md §5.1, and two CPU baselines timed on the host cores (`cpu_baseline`: the
structure-faithful port of the reference's std::list walk, and `fast_cpu`: the closed-form
binary-search window on all cores).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

With --gpus N > 1 and no WORLD_SIZE in the environment, bench.py starts the N ranks itself (one
child process per GPU, before anything touches the GPU) and exits with their status.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "k=8 closest-node queries/sec at 100M-node table (1/8 GPU) + % HBM roofline"
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (AMD's data sheet: 8 TB/s)
LINE_BYTES = {8: 128, 16: 128, 32: 256}  # window line gathered per query
MAX_BATCHES = 128  # default cap on the rotated batches (54 MB each; 128 of them are 27 times the Infinity Cache)
GRAPH_STEPS = 2048  # longest HIP graph: more steps go out as replays of one graph of up to this many launches
DUMP_BYTES = 40_000_000  # --dump-outputs: most it writes per rank (float64 indices, float32 counts: 8 k + 4 bytes per row)
DUMP_SEED = 0x0D470D0  # of the row sample, when a step returns more than that


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--count", type=int, default=8)
    ap.add_argument("--queries", type=int, default=1 << 20, help="queries per GPU per step")
    ap.add_argument("--batches", type=int, default=0,
                    help=f"distinct target batches rotated over the steps (0: one per step, warm-up included, at most "
                         f"{MAX_BATCHES})")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: the check of the last step's rows against the CPU restatement, the "
                         "reference-structure bytes, the CPU baselines, the cold-cache / refresh / host-buffer / "
                         "other-count / latency / config passes, the owner-routed step and the north-star variant "
                         "(--no-cpu, --no-extras, --no-allgather, --no-rccl1 leave parts of it out)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step returned (its rows and counts; a fixed seeded sample of the "
                         f"rows where they would exceed {DUMP_BYTES // 10**6} MB) as DIR/<name>.npy")
    ap.add_argument("--cpu-budget", type=float, default=12.0, help="seconds of port CPU baseline sampling")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-extras", action="store_true",
                    help="headline only: no cold-cache pass, refresh, allgather variant (profiling runs)")
    ap.add_argument("--no-allgather", action="store_true")
    ap.add_argument("--no-graph", action="store_true", help="issue the K steps one by one instead of one HIP graph")
    ap.add_argument("--traffic-json", default=os.path.join(ROOT, "profiles", "traffic_r06.json"))
    ap.add_argument("--gather-json", default=os.path.join(ROOT, "profiles", "r03_mb_gather_nt.json"))
    ap.add_argument("--plumbing", action="store_true",
                    help="launcher/rendezvous check without a GPU: gloo ranks, barrier, max-over-ranks, one line")
    ap.add_argument("--mode", choices=("owner", "allgather", "allgather-child", "owner-child", "rccl1-child"),
                    default="owner",
                    help="owner: the headline (allgather measured as a sub-object); allgather: only the "
                         "north-star variant, as its own line; allgather-child: internal (allgather_child)")
    ap.add_argument("--verify-rows", type=int, default=1 << 16,
                    help="rows of the last timed step checked against the CPU restatement on every rank")
    ap.add_argument("--ag-timeout", type=float, default=240.0,
                    help="seconds before the north-star child processes (N > 1) are killed")
    ap.add_argument("--ag-out", default="", help="internal: where an allgather child writes its result")
    ap.add_argument("--no-rccl1", action="store_true",
                    help="N = 1: skip the one-rank RCCL step (allgather.rccl_world1, a child process)")
    return ap.parse_args(argv)


# ---------------------------------------------------------------------------------------------
# launcher: one process per GPU when not started by torch.distributed.run
# ---------------------------------------------------------------------------------------------
def spawn(args) -> int:
    """Start args.gpus ranks of this script (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set) and wait.
    Nothing here touches the GPU, so the children initialise it themselves."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus),
                   LOCAL_WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rcs = [p.wait() for p in procs]
    bad = [rc for rc in rcs if rc != 0]
    return bad[0] if bad else 0


# Rehearsal of the N-rank flow on a one-GPU box (tests/test_bench_multirank.py): every rank on cuda:0 and gloo
# instead of RCCL (RCCL needs one GPU per rank). Never set by the driver.
REHEARSE_ONE_GPU = os.environ.get("KADGPU_BENCH_ONE_GPU") == "1"


def dist_env():
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local = 0 if REHEARSE_ONE_GPU else int(os.environ.get("LOCAL_RANK", "0"))
    return world, rank, local


def init_dist(world, dev, rccl=False):
    """The process group. The headline (owner routing) has no data-path collective: its barriers and
    max-over-ranks run on gloo, so no RCCL call can stall or fail the headline line. rccl=True (the
    north-star child processes, allgather_child) opens RCCL over xGMI. A finite timeout ends a hung
    collective with an error instead of stalling the run."""
    if world == 1:
        return None
    from datetime import timedelta

    import torch.distributed as dist

    if rccl and dev.type == "cuda" and not REHEARSE_ONE_GPU:
        dist.init_process_group("nccl", device_id=dev, timeout=timedelta(seconds=120))  # RCCL over xGMI
    else:
        dist.init_process_group("gloo", timeout=timedelta(seconds=600))
    return dist


def max_over_ranks(dist, x: float, dev=None) -> float:
    if dist is None:
        return x
    import torch

    t = torch.tensor([x], dtype=torch.float64,
                     device=dev if (dev is not None and dist.get_backend() == "nccl") else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def sum_over_ranks(dist, x: int, dev=None) -> int:
    if dist is None:
        return x
    import torch

    t = torch.tensor([x], dtype=torch.int64,
                     device=dev if (dev is not None and dist.get_backend() == "nccl") else "cpu")
    dist.all_reduce(t)
    return int(t.item())


def host_cores() -> dict:
    """The CPU this process may use: affinity set, cgroup quota, nproc."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        pass
    return {"affinity": aff, "cgroup_quota_cpus": quota, "nproc": os.cpu_count()}


def all_cores() -> int:
    """Threads for the all-cores CPU baseline: the affinity set, capped by the cgroup CPU quota."""
    h = host_cores()
    n = h["affinity"]
    if h["cgroup_quota_cpus"]:
        n = min(n, max(1, int(h["cgroup_quota_cpus"])))
    return max(1, n)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def device_targets(n_batches, q, shard_bits, shard, seed, dev):
    """n_batches x (q, 20) uniform random targets generated on the device; the top shard_bits bits
    of each are forced to `shard` (owner routing: every target is owned by this rank)."""
    import torch

    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    out = []
    for _ in range(n_batches):
        t = torch.randint(0, 256, (q, 20), dtype=torch.uint8, device=dev, generator=g)
        if shard_bits:
            keep = (1 << (8 - shard_bits)) - 1
            t[:, 0] = (t[:, 0] & keep) | (shard << (8 - shard_bits))
        out.append(t)
    return out


def node_times(status, now_ns, seed=0x71E):
    """Node::time / reply_time / expired_ arrays (node.h:39-40,105) that give `status` at now_ns under
    Node::isGood (node.cpp:34-40), shaped like a live table: good nodes were last heard uniformly over the
    last 10 minutes and last replied over the last 120, so their isGood deadlines spread over the next 10
    minutes; expired -> expired_ set; dubious -> last heard 11 minutes ago."""
    n = status.shape[0]
    rng = np.random.default_rng(seed)
    MIN = 60 * 10**9
    t = now_ns - rng.integers(0, 10 * MIN, n, dtype=np.int64)
    rt = now_ns - rng.integers(0, 120 * MIN, n, dtype=np.int64)
    dub = (status & 3) == 0
    t[dub] = now_ns - 11 * MIN
    expired = ((status & 2) != 0).astype(np.uint8)
    return t, rt, expired


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


# ---------------------------------------------------------------------------------------------
# CPU baselines (rank 0, N=1): the oracle is test infrastructure, used here only as the timed
# CPU comparator, never on the GPU path
# ---------------------------------------------------------------------------------------------
def cpu_baselines(sh, targets, count, budget_s, nthreads, min_port=1000, fast_min_s=1.0):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O

    # port: the structure-faithful restatement (std::list buckets, linear findBucket, insertion sort)
    t0 = time.perf_counter()
    F = O.FaithfulTable(sh.ids, sh.status, sh.first, sh.off)
    build_s = time.perf_counter() - t0
    n, dt, chunk = 0, 0.0, max(2 * nthreads, 32)
    while n < targets.shape[0] and (dt < budget_s or n < min_port):
        sl = targets[n:n + chunk]
        t0 = time.perf_counter()
        F.rt_closest(sl, count, nthreads=nthreads)
        dt += time.perf_counter() - t0
        n += sl.shape[0]
        rate = n / max(dt, 1e-9)
        chunk = int(min(4 * chunk, max(2 * nthreads, rate * max(budget_s - dt, 0.5), min_port - n)))
    # the same on one thread (1 thread and all cores), a few seconds of it
    n1, dt1 = 0, 0.0
    while dt1 < budget_s / 3 and n1 < targets.shape[0]:
        t0 = time.perf_counter()
        F.rt_closest(targets[n1:n1 + 4], count, nthreads=1)
        dt1 += time.perf_counter() - t0
        n1 += 4
    F.close()
    port = {"value": n / dt, "unit": "queries/s", "cores": nthreads, "kind": "port",
            "value_1thread": n1 / dt1, "sample_1thread": f"{n1} queries in {dt1:.1f} s on one thread",
            "sample": f"{n} of the {targets.shape[0]} queries of rank 0's first batch (same shard table, "
                      f"{sh.first.shape[0]} buckets, {sh.ids.shape[0]} nodes) in {dt:.1f} s; structure-faithful "
                      f"restatement of routing_table.cpp:67-135 (std::list walk); table build {build_s:.1f}s excluded",
            "cpu_model": cpu_model(), "host": host_cores()}
    # fast_cpu: the closed-form window (binary-search findBucket, good counts, sort), all cores; passes over
    # the whole host sample until at least fast_min_s of CPU work is timed
    O.flat_rt_closest(sh.ids, sh.status, sh.first, sh.off, targets[:4096], count, nthreads=nthreads)  # warm pages
    fq, fdt, passes = 0, 0.0, 0
    while fdt < fast_min_s:
        t0 = time.perf_counter()
        O.flat_rt_closest(sh.ids, sh.status, sh.first, sh.off, targets, count, nthreads=nthreads)
        fdt += time.perf_counter() - t0
        fq += targets.shape[0]
        passes += 1
    t0 = time.perf_counter()
    O.flat_rt_closest(sh.ids, sh.status, sh.first, sh.off, targets[:1 << 14], count, nthreads=1)
    fdt1 = time.perf_counter() - t0
    fast = {"value": fq / fdt, "unit": "queries/s", "cores": nthreads, "kind": "port",
            "value_1thread": (1 << 14) / fdt1, "sample_1thread": f"{1 << 14} queries in {fdt1:.2f} s on one thread",
            "sample": f"{passes} passes over {targets.shape[0]} queries of rank 0's first batch ({fq} queries) in "
                      f"{fdt:.2f} s; closed-form flat restatement "
                      f"(upper_bound findBucket + window rounds + sort by XOR distance), {nthreads} threads",
            "cpu_model": cpu_model(), "host": host_cores()}
    return port, fast


def verify_rows(ids, status, first, off, index_base, targets, idx, cnt, count, nthreads=None) -> int:
    """Rows of a timed step against the closed-form CPU restatement (oracle/, the checker) on the same
    table: the number of rows whose indices or count differ."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O

    if targets.shape[0] == 0:
        return 0
    want, wcnt = O.flat_rt_closest(ids, status, first, off, targets, count, nthreads=nthreads or all_cores())
    want = np.where(want != 0xFFFFFFFF, want + np.uint32(index_base), want)
    got = np.ascontiguousarray(idx).view(np.uint32).reshape(want.shape)
    return int(((got != want).any(axis=1) | (np.asarray(cnt) != wcnt)).sum())


def load_json(path, key=None):
    try:
        d = json.load(open(path))
    except (OSError, ValueError):
        return None
    return d.get(key) if key else d


def dump_outputs(path, idx, cnt, world=1, rank=0):
    """--dump-outputs: what the last timed step returned to its caller, as path/idx.npy (the rows: global node
    indices, -1 where a row has fewer, float64 so that every index is exact) and path/cnt.npy (the rows' counts,
    float32); at N > 1 every rank writes its own pair, named idx_rank<r> / cnt_rank<r>. A step returning more than
    DUMP_BYTES has a fixed sample of its rows written (the same rows in every run: DUMP_SEED, in ascending order)."""
    n = idx.shape[0]
    keep = DUMP_BYTES // (8 * idx.shape[1] + 4)
    tag = f"_rank{rank}" if world > 1 else ""
    os.makedirs(path, exist_ok=True)
    i, c = idx.cpu().numpy(), cnt.cpu().numpy()
    if n > keep:
        rows = np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=keep, replace=False))
        i, c = i[rows], c[rows]
    np.save(os.path.join(path, f"idx{tag}.npy"), i.astype(np.float64))
    np.save(os.path.join(path, f"cnt{tag}.npy"), c.astype(np.float32))


# ---------------------------------------------------------------------------------------------
# owner routing (the headline)
# ---------------------------------------------------------------------------------------------
def main_owner(args):
    import torch

    from opendht_amd import DeviceTable
    from opendht_amd._lib import KAD_INFO_SHORT_LINES, KAD_INFO_WINDOW_LINES
    from opendht_amd.metrics import rt_algorithmic_bytes
    from opendht_amd.sharded import build_shard, config3_spec

    world, rank, local = dist_env()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if world > 8:
        raise SystemExit("the 100M-node table has 8 shards: at most 8 GPUs")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = init_dist(world, dev)

    spec = config3_spec()  # SURVEY §8d's 100M-node U(24) table, 8 shards, k_max 32
    t0 = time.perf_counter()
    sh = build_shard(spec, rank)
    T = DeviceTable(sh.ids, sh.status, sh.first, sh.off, device=local, index_base=sh.index_base, sorted=True)
    Q, K, W, cnt_k = args.queries, args.steps, args.warmup, args.count
    if K < 1 or W < 0:
        raise SystemExit("--steps must be at least 1 and --warmup at least 0")
    NB = args.batches or min(K + W, MAX_BATCHES)
    tgs = device_targets(NB, Q, spec.shard_bits, rank, 0x0D470002 + 7919 * rank, dev)
    outs = [torch.empty((Q, cnt_k), dtype=torch.int32, device=dev) for _ in range(NB)]
    ocnt = [torch.empty((Q,), dtype=torch.uint8, device=dev) for _ in range(NB)]
    setup_s = time.perf_counter() - t0
    stream = torch.cuda.current_stream(dev)
    flags = T.info()["flags"]
    wl = bool(flags & KAD_INFO_WINDOW_LINES)  # the shard's U(24) table carries every line set
    kk = 8 if cnt_k <= 8 else 16 if cnt_k <= 16 else 32
    ws = kk == 8 and bool(flags & KAD_INFO_SHORT_LINES) and os.environ.get("KAD_RT_KERNEL") not in ("wl", "lane")
    kernel = ("rt_ws_kernel<0, true, true>" if ws else {8: "rt_wl_kernel<0>", 16: "rt_wl16_kernel<0>", 32: "rt_wl32_kernel"}[kk]
              if wl else f"rt_closest_kernel<{kk}>")
    line_b = 64 if ws else LINE_BYTES[kk]

    def step(j, s):
        T.rt_closest(tgs[j % NB], cnt_k, outs[j % NB], ocnt[j % NB], stream=s)

    for j in range(W):
        step(K + j, stream.cuda_stream)
    torch.cuda.synchronize(dev)

    # The K steps go out as one HIP graph of K launches (a step is ~30 us; issuing them one by one
    # from Python leaves ~3 us gaps). Step j reads batch j % NB and writes output j % NB. More than GRAPH_STEPS
    # steps go out as replays of one graph of C launches (C a multiple of NB, so every replay starts at batch 0)
    # and one graph of the K % C steps left. --no-graph issues them one by one with an event per step.
    C = K if K <= GRAPH_STEPS else NB * max(1, GRAPH_STEPS // NB)
    graph = None
    if not args.no_graph:
        try:
            graph = []  # (graph, replays)
            cs = torch.cuda.Stream(dev)
            for j0, n, replays in ((0, C, K // C), (K - K % C, K % C, 1)):
                if n == 0:
                    continue
                g = torch.cuda.CUDAGraph()
                cs.wait_stream(stream)
                with torch.cuda.graph(g, stream=cs):
                    for j in range(j0, j0 + n):
                        step(j, cs.cuda_stream)
                stream.wait_stream(cs)
                torch.cuda.synchronize(dev)
                graph.append((g, replays))
        except Exception as e:  # capture unsupported: fall back to eager launches
            print(f"graph capture failed ({e}); eager launches", file=sys.stderr)
            graph = None
    if graph is not None:  # a graph's first launch uploads it: run each once untimed over the warm-up
        for g, _ in graph:
            g.replay()
        for j in range(W):
            step(K + j, stream.cuda_stream)
        torch.cuda.synchronize(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 if graph is not None else K + 1)]
    if dist:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t_start = time.perf_counter()
    ev[0].record(stream)
    if graph is not None:
        for g, replays in graph:
            for _ in range(replays):
                g.replay()
        ev[-1].record(stream)
    else:
        for j in range(K):
            step(j, stream.cuda_stream)
            ev[j + 1].record(stream)
    torch.cuda.synchronize(dev)
    if dist:
        dist.barrier()
    wall = time.perf_counter() - t_start
    if graph is not None:
        kern_ms = [ev[0].elapsed_time(ev[-1]) / K]
    else:
        kern_ms = [ev[j].elapsed_time(ev[j + 1]) for j in range(K)]
    t_max = max_over_ranks(dist, wall, dev)
    avg_kernel_s = float(np.mean(kern_ms)) / 1e3
    if args.dump_outputs:  # (before the passes below, which reuse the buffers)
        dump_outputs(args.dump_outputs, outs[(K - 1) % NB], ocnt[(K - 1) % NB], world, rank)

    # bytes the timed kernel must move per query: the target, its ONE window line, the row and count
    moved_q = 20 + line_b + 4 * cnt_k + 1
    achieved = moved_q * Q / avg_kernel_s / 1e9
    # --full: SURVEY §8(d)'s reference-structure bytes (IDs of every good node of W(R), status bytes, extents)
    # over the first batches, exact on the host; reported without a fraction (the layout reads less)
    ref_structure = None
    if args.full:
        ref = [rt_algorithmic_bytes(sh.status, sh.off, T.find_bucket(tgs[j]).cpu().numpy().view(np.uint32)
                                    .astype(np.int64), cnt_k) for j in range(min(4, NB))]
        ref_structure = {
            "bytes_per_query": float(np.mean([r[0] for r in ref])) / Q,
            "basis": "SURVEY.md §8(d): 20 + sum over W(R) of (8 + n_b + 20 g_b) + 4k, the bytes the "
                     "reference's own data structure must read (no fraction: the window lines read less)",
            "window_means": {"buckets": float(np.mean([r[1] for r in ref])),
                             "nodes": float(np.mean([r[2] for r in ref])),
                             "good": float(np.mean([r[3] for r in ref]))},
        }
    traffic = traffic_src = None
    tj = load_json(args.traffic_json)
    if tj and tj.get("kernel", "") in kernel and tj.get("count") == cnt_k:
        traffic = tj.get("hbm_bytes_per_launch")
        traffic_src = {"file": os.path.relpath(args.traffic_json, ROOT), "date": tj.get("date"),
                       "source": tj.get("source"), "correction": tj.get("correction"),
                       "note": "rocprofv3 PMC of a separate run of this command (counters cannot be collected in the "
                               "timed run); not measured by this run"}
    gath = load_json(args.gather_json)
    # the ceiling row for this line size and table footprint (64-byte lines: 134 MB; 128-byte: 268 MB)
    ceil = None
    if gath and line_b in (64, 128):
        row = "128MB_64B" if line_b == 64 else "256MB_128B"
        a = gath.get("all", {})
        if row in a and row + "_cold" in a:
            ceil = {"what": f"random {line_b}-byte line gather + 20 B target read + 32 B row write per query (the "
                            "streams non-temporal, as the kernel's), 1M queries per launch, rotated batches "
                            "(tools/mb_gather_nt.py)",
                    "table_MB": int(row.split("MB")[0]), "line_bytes": line_b,
                    "us_per_1M_rotated": a[row]["us_per_1M"], "us_per_1M_cold": a[row + "_cold"]["us_per_1M"]}

    # --full: the rows of the last timed step (batch K-1; before the extras, which reuse the buffers and change the
    # status), checked against the CPU restatement on this rank's
    # shard table (exact halo: every owned window lies inside it)
    verified = None
    if args.full:
        vrows = min(Q, args.verify_rows)
        vt = tgs[(K - 1) % NB][:vrows].cpu().numpy()
        bad = verify_rows(sh.ids, sh.status, sh.first, sh.off, sh.index_base, vt,
                          outs[(K - 1) % NB][:vrows].cpu().numpy(), ocnt[(K - 1) % NB][:vrows].cpu().numpy(), cnt_k)
        verified = {"rows": sum_over_ranks(dist, vrows), "mismatches": sum_over_ranks(dist, bad),
                    "what": f"the first {vrows} rows (indices, counts) of every rank's last timed step, against the "
                            "closed-form CPU restatement (oracle/) on the rank's shard table"}
    extras = {}
    if args.full and not args.no_extras:
        extras["cold"] = cold_pass(T, tgs, outs, ocnt, cnt_k, Q, moved_q, dev, stream)
        # (before refresh_pass, which moves `now` and so the statuses the rows are checked against)
        # N > 1: in child processes whose data path runs on an RCCL group (owner_child); N = 1: no exchange here,
        # and the same pass through a one-rank RCCL group in the rccl1 child (owner_routed.rccl_world1)
        extras["owner_routed"] = (owner_routed_pass(T, sh, spec, Q, cnt_k, K, W, dev, dist, world, rank) if world == 1
                                  else owner_child(args, world, rank, local, dist))
        extras["refresh"] = refresh_pass(T, sh, tgs, outs, ocnt, cnt_k, Q, avg_kernel_s, dev, stream)
        extras["host_buffers"] = host_pass(T, tgs, cnt_k, Q, dev)
        extras["other_counts"] = counts_pass(T, tgs, Q, dev, stream)
        if rank == 0:
            try:
                extras["owner_step_model"] = owner_step_model(T, Q, cnt_k, dev, stream, avg_kernel_s)
            except Exception as e:  # a model, never the line's failure
                extras["owner_step_model"] = {"error": f"{type(e).__name__}: {e}"}
        if rank == 0:
            extras["latency"] = latency_pass(dev)
        if rank == 0 and world == 1:
            extras["configs"] = configs_pass(dev)
    cpu = fast = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu:
        host_t = tgs[0][:1 << 17].cpu().numpy()
        cpu, fast = cpu_baselines(sh, host_t, cnt_k, args.cpu_budget, all_cores())
    ag = None
    if args.full and not args.no_extras and not args.no_allgather:
        T.close()
        del tgs, outs, ocnt
        torch.cuda.empty_cache()
        if world == 1:
            try:
                ag = allgather_pass(args, world, rank, local, dev, None)
            except Exception as e:  # the headline line is printed whatever happens here
                ag = {"error": f"{type(e).__name__}: {e}"}
        else:
            ag = allgather_child(args, world, rank, local, dist)

    if isinstance(ag, dict) and isinstance(ag.get("rccl_world1"), dict) and "owner_routed" in ag["rccl_world1"]:
        ow = extras.get("owner_routed")
        if isinstance(ow, dict):
            ow["rccl_world1"] = ag["rccl_world1"].pop("owner_routed")
    if rank == 0:
        line = {
            "metric": METRIC,
            "value": world * Q * K / t_max,
            "unit": "queries/s",
            "n_gpus": world,
            "steps": K,
            "warmup": W,
            "ms_per_step": t_max / K * 1e3,
            "full": bool(args.full),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u64",
            "data": "synthetic (SURVEY.md §8d recipe: 100M mt19937_64 IDs, seed 0x0D470001, status 80/10/10 "
                    "good/expired/dubious from seed 0x0D470003, U(24) buckets; uniform targets, "
                    f"{NB} distinct batches of {Q} per GPU, "
                    f"{'one per step' if NB >= K + W else 'rotated over the steps'})",
            "config": {
                "workload": "config3: 100M-node U(24) routing table, 1/8 shard per GPU (2^21 owned buckets "
                            f"+ halo, {sh.ids.shape[0]} nodes on rank 0), {Q} owned queries per GPU "
                            f"per step, k={cnt_k}, a distinct target batch and output buffer per step",
                "table_nodes_per_gpu": int(sh.ids.shape[0]),
                "buckets_per_gpu": int(sh.first.shape[0]),
                "queries_per_gpu": Q,
                "k": cnt_k,
                "parallelism": f"id-range shards x{world}, owner routing (no data-path collective)",
            },
            "roofline": {
                "bound": "hbm",
                "achieved": achieved,
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                "traffic": traffic,
                "traffic_source": traffic_src,
                "kernel": kernel,
                "bytes_per_query": moved_q,
                "bytes_basis": f"bytes the kernel must move per query: 20 target + {line_b} window line "
                               f"+ {4 * cnt_k} row + 1 count (the 128-byte fallback lines and exact-path reads of "
                               "the rare queries that need them not counted)",
                "launch": ("K eager launches" if graph is None else "hip graph of K launches" if C == K
                           else f"replays of a hip graph of {C} launches"),
                "avg_kernel_ms": avg_kernel_s * 1e3,
                "random_line_ceiling": ceil,
                "frac_of_ceiling": (ceil["us_per_1M_rotated"] * Q / 2**20 / 1e3 / (avg_kernel_s * 1e3)) if ceil else None,
                "alg_bytes_ref_structure": ref_structure,
            },
            "verified": verified,
            "cpu_baseline": cpu,
            "fast_cpu": fast,
            "setup_s": setup_s,
        }
        line.update(extras)
        if ag is not None:
            line["allgather"] = ag
        print(json.dumps(line), flush=True)
    if dist:
        dist.barrier()
        dist.destroy_process_group()


def data_backend(world: int, dev) -> str | None:
    """The backend of owner routing's data-path group (the all_to_alls of the target blocks and the rows): RCCL over
    xGMI whenever the ranks have a GPU each (world > 1 on CUDA devices); gloo only in the one-GPU rehearsal
    (KADGPU_BENCH_ONE_GPU, every rank on cuda:0) and on CPU; none at world 1."""
    if world <= 1:
        return None
    return "nccl" if dev.type == "cuda" and not REHEARSE_ONE_GPU else "gloo"


def verify_routed(dist, sh, spec, rank, world, tg, idx, cnt, cnt_k, rows=65536) -> dict:
    """Rows that came back through owner routing, checked by the ranks that own them: every rank's first `rows`
    (target, row, count) triples are all-gathered over the default group (gloo, host tensors), and each rank checks
    the triples whose target it owns against the CPU restatement (oracle/) on its own shard table. So the rows answered
    by another rank and returned over the links ((N-1)/N of them) are checked as well as the rank's own."""
    import torch

    v = min(rows, tg.shape[0])
    rec = np.concatenate([tg[:v].cpu().numpy(), idx[:v].cpu().numpy().view(np.uint8).reshape(v, -1),
                          cnt[:v].cpu().numpy().reshape(v, 1)], axis=1)
    src = np.full(v, rank, np.int64)
    if world > 1:
        parts = [torch.empty(rec.shape, dtype=torch.uint8) for _ in range(world)]
        dist.all_gather(parts, torch.from_numpy(np.ascontiguousarray(rec)))
        rec = np.concatenate([p.numpy() for p in parts])
        src = np.repeat(np.arange(world), v)
    own = (rec[:, 0].astype(np.int64) >> (8 - spec.shard_bits)) == rank if spec.shard_bits else np.ones(len(rec), bool)
    r = rec[own]
    bad = verify_rows(sh.ids, sh.status, sh.first, sh.off, sh.index_base, np.ascontiguousarray(r[:, :20]),
                      np.ascontiguousarray(r[:, 20:20 + 4 * cnt_k]).view(np.int32),
                      np.ascontiguousarray(r[:, 20 + 4 * cnt_k]), cnt_k)
    cross = int((src[own] != rank).sum())
    if world == 1:
        dist = None  # (a one-rank group: nothing to sum)
    return {"rows": sum_over_ranks(dist, int(own.sum())), "mismatches": sum_over_ranks(dist, bad),
            "rows_answered_by_another_rank": sum_over_ranks(dist, cross),
            "what": f"the first {v} rows of every rank's last batch, all-gathered; each row checked by the rank owning "
                    "its target against the CPU restatement on that rank's shard table"}


def routed_targets(Q, world, rank, dev, NB, seed=0x0D470600):
    """NB batches of Q arbitrary targets per rank, spread uniformly over the `world` shards of the 8-shard layout's
    first `world` shards (top three bits = a random rank < world)."""
    import torch

    g = torch.Generator(device=dev)
    g.manual_seed(seed + rank)
    tgs = []
    for _ in range(NB):
        t = torch.randint(0, 256, (Q, 20), dtype=torch.uint8, device=dev, generator=g)
        own = torch.randint(0, world, (Q,), dtype=torch.int32, device=dev, generator=g)
        t[:, 0] = ((t[:, 0].to(torch.int32) & 0x1F) | (own << 5)).to(torch.uint8)
        tgs.append(t)
    return tgs


def owner_routed_pass(T, sh, spec, Q, cnt_k, K, W, dev, dist, world, rank, NB=4, group=None, collective=None,
                      pipelined=None, comm=None):
    """The headline form as a serving front end, measured at this N: every rank holds Q arbitrary
    targets per step (uniform over the N shards), routes each to its owner and gets the rows back
    (sharded.OwnerRoute.step: kad_route_pack, all_to_all_single of the target blocks on `group` — RCCL over xGMI at
    N > 1 —, the owner's kad_rt_closest_batch_packed over the blocks it received, all_to_all_single of the packed
    rows back, kad_route_unpack_packed). W + K eager steps (collectives are not captured), barrier + synchronize on
    both sides, the max over ranks; a distinct batch per step (NB rotated); each step's overflow and escape words
    folded on the device and read once after. `pipelined`: the same K batches through sharded.OwnerPipeline (batch
    i's exchanges on a comm stream under batch i+1's pack and batch i's answer). `comm` (an opendht_amd.comm.Comm):
    the same batches through the native executor too (native_pass). At N = 1 without `collective` there is no
    exchange (the local pack / query / unpack)."""
    import torch

    from opendht_amd.sharded import OwnerRoute

    want = data_backend(world, dev)
    coll = world > 1 if collective is None else bool(collective)
    if world > 1 and dist.get_backend(group) != want:
        raise RuntimeError(f"owner routing's data path must run on {want} at N = {world} "
                           f"(got {dist.get_backend(group)})")
    if pipelined is None:
        pipelined = coll
    try:
        tgs = routed_targets(Q, world, rank, dev, NB)
        s = torch.cuda.current_stream(dev).cuda_stream
        R = OwnerRoute(Q, cnt_k, world, spec.shard_bits, dev, collective=coll)
        outs = [(torch.empty((Q, cnt_k), dtype=torch.int32, device=dev), torch.empty((Q,), dtype=torch.uint8, device=dev))
                for _ in range(NB)]
        acc = torch.zeros((3,), dtype=torch.int32, device=dev)
        for _ in range(6):  # block capacities: grow until a step fits (decided together over the ranks)
            R.step(T, tgs[0], *outs[0], group, s)
            if not R.overflowed(group):
                break
            R = R.grown(group)

        def step(j):
            R.step(T, tgs[j % NB], *outs[j % NB], group, s)
            R.fold_flags(acc, s)

        t_max, ev_ms, how = graph_steps(step, K, W, dev, dist, use_graph=False)
        from opendht_amd.sharded import combine_max

        over, esc, tail = (bool(x) for x in combine_max(acc, group, coll))
        last = (K - 1) % NB
        if tail or esc:  # (some step needed full targets or unpacked rows: the last batch again, that way)
            R.step(T, tgs[last], *outs[last], group, s, packed=not esc, keys=False)
            torch.cuda.synchronize(dev)
        verified = verify_routed(dist, sh, spec, rank, world, tgs[last], *outs[last], cnt_k)
        xb = R.xgmi_bytes
        backend = dist.get_backend(group) if coll else None
        res = {"queries_per_s": world * Q * K / t_max, "ms_per_step": t_max / K * 1e3, "n_gpus": world,
               "collective": (f"all_to_all_single ({'RCCL' if backend == 'nccl' else backend})" if coll else None),
               "cap": R.cap, "overflow": over,
               "targets_out": f"{R.record_bytes} bytes per query" + (" (key-only: the top 64 bits)" if R.keys else ""),
               "rows_back": f"packed, {4 * R.pw} bytes per row" if R.packed else "plain", "escaped": esc,
               "tailed": tail,
               "xgmi_bytes_per_rank_step": xb, "launch": how, "verified": verified,
               "how": owner_routed_pass.__doc__.split("\n\n")[0].replace("\n", " ")}
        if pipelined:
            res["pipelined"] = pipelined_pass(T, sh, spec, tgs, outs, Q, cnt_k, K, W, dev, dist, world, rank, R.cap,
                                              group, coll)
        if comm is not None:
            try:
                res["native"] = native_pass(T, sh, spec, tgs, outs, Q, cnt_k, K, W, dev, dist, world, rank, R.cap,
                                            comm, group)
            except Exception as e:
                res["native"] = {"error": f"{type(e).__name__}: {e}"}
        return res
    except Exception as e:  # the headline line is printed whatever happens here
        return {"error": f"{type(e).__name__}: {e}"}


def issue_timed(issue, K, dev, dist, graph_ok):
    """Time K batches issued by issue(): eager (the wall time and the host's issue time alone), then — when graph_ok
    (RCCL or no collective: gloo stages through the host and cannot be captured) — the same issue captured once as
    one HIP graph (fork/join of the compute and comm streams by events, the RCCL collectives as graph nodes) and
    replayed. Barrier + synchronize on both sides, max over ranks. Returns {mode: (max wall s, host issue s)}."""
    import torch

    out = {}
    if dist:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    issue()
    t1 = time.perf_counter()
    torch.cuda.synchronize(dev)
    if dist:
        dist.barrier()
    out["eager"] = (max_over_ranks(dist, time.perf_counter() - t0, dev), max_over_ranks(dist, t1 - t0, dev))
    if graph_ok:
        try:
            g = torch.cuda.CUDAGraph()
            cur = torch.cuda.current_stream(dev)
            cap = torch.cuda.Stream(dev)
            cap.wait_stream(cur)
            with torch.cuda.graph(g, stream=cap):
                issue()
            cur.wait_stream(cap)
            g.replay()  # the first replay uploads the graph
            torch.cuda.synchronize(dev)
            if dist:
                dist.barrier()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            g.replay()
            torch.cuda.synchronize(dev)
            if dist:
                dist.barrier()
            out["graph"] = (max_over_ranks(dist, time.perf_counter() - t0, dev), 0.0)
            del g
        except Exception as e:
            out["graph_error"] = f"{type(e).__name__}: {e}"
    return out


def pipelined_pass(T, sh, spec, tgs, outs, Q, cnt_k, K, W, dev, dist, world, rank, cap, group, coll):
    """owner_routed_pass's K batches through sharded.OwnerPipeline (three buffer sets, compute and comm streams): the
    same barrier + synchronize on both sides and max over ranks, the overflow / escape words folded on the device
    and combined after; eager (with the host's issue time) and as one HIP graph of the K batches; the last batch's
    rows checked by their owners."""
    import torch

    from opendht_amd.sharded import OwnerPipeline

    NB = len(tgs)
    P = OwnerPipeline(Q, cnt_k, world, spec.shard_bits, dev, cap=cap, collective=coll)
    for _ in range(6):
        P.run(T, tgs[:2], outs[:2], group)
        over, esc, tail = P.flags(group)
        if not over:
            break
        P = P.grown(group)
    P.run(T, [tgs[j % NB] for j in range(W)], [outs[j % NB] for j in range(W)], group)
    torch.cuda.synchronize(dev)
    P.flags(group)
    # (no HIP graph around the torch RCCL collectives: capturing them crashed the one-rank RCCL child on this image,
    # gpurun_out/r06b; the native executor, kad_comm, issues the pipeline from C++ instead)
    tm = issue_timed(lambda: P.run(T, [tgs[j % NB] for j in range(K)], [outs[j % NB] for j in range(K)], group), K,
                     dev, dist, graph_ok=not coll)
    over, esc, tail = P.flags(group)
    last = (K - 1) % NB
    if tail or esc:
        P.run(T, [tgs[last]], [outs[last]], group, packed=not esc, keys=False)
        torch.cuda.synchronize(dev)
        P.flags(group)
    best = "graph" if "graph" in tm else "eager"
    t_max = tm[best][0]
    res = {"queries_per_s": world * Q * K / t_max, "ms_per_step": t_max / K * 1e3, "launch": best,
           "eager_ms_per_step": tm["eager"][0] / K * 1e3, "eager_host_issue_ms_per_step": tm["eager"][1] / K * 1e3,
           "cap": P.cap, "overflow": over, "escaped": esc, "tailed": tail,
           "verified": verify_routed(dist, sh, spec, rank, world, tgs[last], *outs[last], cnt_k),
           "how": OwnerPipeline.__doc__.split("\n\n")[0].replace("\n", " ")}
    if "graph_error" in tm:
        res["graph_error"] = tm["graph_error"]
    return res


def native_pass(T, sh, spec, tgs, outs, Q, cnt_k, K, W, dev, dist, world, rank, cap, comm, group):
    """owner_routed_pass's K batches through the native executor (opendht_amd.comm.NativeRoute, kad_route_run over the
    engine's own RCCL communicator, one C call per run of batches): `serial` (one buffer set, each batch in order on
    one stream) and `pipelined` (three sets: batch i+1's pack and batch i's query on the compute stream while batch i's
    targets and batch i-1's rows are on the links). Barrier + synchronize on both sides, max over ranks; the host's
    issue time beside; the last batch's rows checked by their owners."""
    import torch

    from opendht_amd.comm import NativeRoute

    NB = len(tgs)
    res = {}
    for name, n_sets in (("serial", 1), ("pipelined", 3)):
        R = NativeRoute(Q, cnt_k, world, spec.shard_bits, dev, cap=cap, n_sets=n_sets, comm=comm)
        for _ in range(6):
            R.run(T, tgs[:2], outs[:2])
            over, esc, tail = R.flags(group)
            if not over:
                break
            R = R.grown(group)
        R.run(T, [tgs[j % NB] for j in range(W)], [outs[j % NB] for j in range(W)])
        torch.cuda.synchronize(dev)
        R.flags(group)
        tm = issue_timed(lambda: R.run(T, [tgs[j % NB] for j in range(K)], [outs[j % NB] for j in range(K)]), K, dev,
                         dist, graph_ok=False)
        over, esc, tail = R.flags(group)
        last = (K - 1) % NB
        if tail or esc:
            R.run(T, [tgs[last]], [outs[last]], packed=not esc, keys=False)
            torch.cuda.synchronize(dev)
            R.flags(group)
        t_max, host = tm["eager"]
        res[name] = {"queries_per_s": world * Q * K / t_max, "ms_per_step": t_max / K * 1e3,
                     "host_issue_ms_per_step": host / K * 1e3, "cap": R.cap, "overflow": over, "escaped": esc,
                     "tailed": tail, "targets_bytes_per_query": 8 if R.keys else 20,
                     "verified": verify_routed(dist, sh, spec, rank, world, tgs[last], *outs[last], cnt_k)}
        del R
    res["how"] = native_pass.__doc__.split("\n\n")[0].replace("\n", " ")
    return res


def owner_step_model(T, Q, cnt_k, dev, stream, avg_kernel_s, link_gbs=64.0, lat_us=10.0, reps=20):
    """The headline form's multi-GPU data path priced: a serving front end holding Q arbitrary
    targets per rank at N = 2, 4, 8 routes each to the rank owning its shard and gets the rows back
    (sharded.OwnerRoute). Timed on this GPU, on rank 0's shard table: kad_route_pack of Q targets spread over the N
    shards into N blocks, the query over the N blocks rank 0 receives (N x cap owned targets, cap = Q / N + 6 sigma +
    256), kad_route_unpack of the rows. Modelled: the two all_to_all_single exchanges, each rank sending one block
    to every other rank over its own xGMI link at link_gbs GB/s, lat_us per collective (targets: one; rows and
    counts: two). serial = pack + targets + query + rows + unpack; overlapped = the compute and the exchanges of
    consecutive batches on two streams, max(pack + query + unpack, exchanges). `packed`: the same with the rows
    back packed (written packed by the query kernel at count 8 — kad_rt_closest_batch_packed —, by kad_route_compress
    otherwise; one collective of KAD_ROUTE_PACKED_WORDS(k) words per row; kad_route_unpack_packed). `keys` (count 8,
    the default route): the targets out as 8-byte keys, the rows back packed (20 bytes per query on the links instead
    of 32), the kernels as the native executor issues them (kad_route_pack_ex without a memset,
    kad_rt_closest_keys_packed, kad_route_unpack_packed_fold)."""
    import torch

    from opendht_amd.sharded import OwnerRoute

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        fn()
        torch.cuda.synchronize(dev)
        a.record(stream)
        for _ in range(reps):
            fn()
        b.record(stream)
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / reps * 1e3

    g = torch.Generator(device=dev)
    g.manual_seed(0x0D470777)
    s = stream.cuda_stream
    out = {"link_GBps_assumed": link_gbs, "latency_us_per_collective_assumed": lat_us, "queries_per_rank": Q,
           "headline_kernel_us": avg_kernel_s * 1e6}
    for n in (2, 4, 8):
        t = torch.randint(0, 256, (Q, 20), dtype=torch.uint8, device=dev, generator=g)
        sh = torch.randint(0, n, (Q,), dtype=torch.uint8, device=dev, generator=g)
        t[:, 0] = (t[:, 0] & 0x1F) | (sh << 5)  # targets spread over the N held shards of the 8-shard table
        R = OwnerRoute(Q, cnt_k, n, 3, dev, collective=False, keys=False)
        pack_us = timed(lambda: R.pack(t, s))
        over = R.overflowed(combine=False)
        recv = torch.randint(0, 256, (n * R.cap, 20), dtype=torch.uint8, device=dev, generator=g)
        recv[:, 0] &= 0x1F  # what rank 0 receives: targets of its own shard
        query_us = timed(lambda: T.rt_closest(recv, cnt_k, out_idx=R.rows, out_cnt=R.cnt, stream=s))
        oi = torch.empty((Q, cnt_k), dtype=torch.int32, device=dev)
        oc = torch.empty((Q,), dtype=torch.uint8, device=dev)
        unpack_us = timed(lambda: R.unpack(oi, oc, s))
        x_t = lat_us + 20 * R.cap / (link_gbs * 1e3)
        x_r = 2 * lat_us + (4 * cnt_k + 1) * R.cap / (link_gbs * 1e3)
        serial = pack_us + x_t + query_us + x_r + unpack_us
        overlap = max(pack_us + query_us + unpack_us, x_t + x_r)
        e = {"cap": R.cap, "overflow": over, "pack_us": pack_us, "query_us": query_us,
             "unpack_us": unpack_us, "xgmi_targets_bytes": 20 * (n - 1) * R.cap,
             "xgmi_rows_bytes": (4 * cnt_k + 1) * (n - 1) * R.cap,
             "exchange_targets_modelled_us": x_t, "exchange_rows_modelled_us": x_r,
             "step_serial_us": serial, "step_overlapped_us": overlap,
             "aggregate_queries_per_s_serial": n * Q / (serial * 1e-6),
             "aggregate_queries_per_s_overlapped": n * Q / (overlap * 1e-6)}
        if R.packed:  # the rows back packed: one collective of packed rows + kad_route_unpack_packed
            R.send, R.recv = recv, recv  # (answer() reads the received block from recv)
            query_p_us = timed(lambda: R.answer(T, s))  # count 8: the query kernel writes packed rows
            fused = R.fused
            compress_us = 0.0 if fused else timed(lambda: R.compress(s))
            esc = R.escaped(combine=False)
            unpack_p_us = timed(lambda: R.unpack_packed(oi, oc, s))
            x_p = lat_us + 4 * R.pw * R.cap / (link_gbs * 1e3)
            qp = (query_p_us if fused else query_us) + compress_us
            serial_p = pack_us + x_t + qp + x_p + unpack_p_us
            overlap_p = max(pack_us + qp + unpack_p_us, x_t + x_p)
            e["packed"] = {"row_bytes": 4 * R.pw, "escaped": esc,
                           "query_us": query_p_us if fused else None, "fused": fused,
                           "compress_us": compress_us, "unpack_us": unpack_p_us,
                           "xgmi_rows_bytes": 4 * R.pw * (n - 1) * R.cap,
                           "exchange_rows_modelled_us": x_p, "step_serial_us": serial_p,
                           "step_overlapped_us": overlap_p,
                           "aggregate_queries_per_s_serial": n * Q / (serial_p * 1e-6),
                           "aggregate_queries_per_s_overlapped": n * Q / (overlap_p * 1e-6)}
            if cnt_k == 8:  # key-only targets (8 bytes out) + packed rows (12 back): kad_route_pack_keys,
                # kad_rt_closest_keys_packed, kad_route_unpack_packed
                import ctypes as C

                from opendht_amd._lib import KAD_ROUTE_KEYS, KAD_ROUTE_ZEROED, check, lib, ptr, route_ctr_words

                RK = OwnerRoute(Q, cnt_k, n, 3, dev, collective=False, keys=True)
                # as the native executor runs them (kad_route_run): the pack without a memset (KAD_ROUTE_ZEROED, a
                # fresh zeroed counter set per launch), the unpack folding and zeroing the counters in its launch
                cw = route_ctr_words(n)
                ctrs = torch.zeros((reps + 1, cw), dtype=torch.int32, device=dev)
                flags = torch.zeros((4,), dtype=torch.int32, device=dev)
                it = iter(range(10**9))

                def pack_z():
                    j = next(it) % (reps + 1)
                    check(lib().kad_route_pack_ex(ptr(t), Q, n, 3, RK.cap, ptr(RK.send_keys), ptr(RK.slot),
                                                  ptr(ctrs[j]), KAD_ROUTE_KEYS | KAD_ROUTE_ZEROED, dev.index or 0,
                                                  C.c_void_p(s)), "kad_route_pack_ex")

                pack_k_us = timed(pack_z)
                RK.recv_keys = recv[:, :8].flip(1).contiguous().view(torch.int64).view(-1)  # big-endian top 64 bits
                query_k_us = timed(lambda: RK.answer(T, s))
                tail = RK.tailed(combine=False)
                RK.back_prow = R.prow  # (rows of the packed answer above: the unpack's input)

                def unpack_f():
                    check(lib().kad_route_unpack_packed_fold(ptr(RK.slot), Q, cnt_k, ptr(RK.back_prow), ptr(oi),
                                                             ptr(oc), ptr(RK.ctr), n, ptr(flags), dev.index or 0,
                                                             C.c_void_p(s)), "kad_route_unpack_packed_fold")

                unpack_k_us = timed(unpack_f)
                x_k = lat_us + 8 * RK.cap / (link_gbs * 1e3)
                serial_k = pack_k_us + x_k + query_k_us + x_p + unpack_k_us
                overlap_k = max(pack_k_us + query_k_us + unpack_k_us, x_k + x_p)
                e["keys"] = {"target_bytes": 8, "row_bytes": 4 * R.pw, "tailed": tail, "pack_us": pack_k_us,
                             "query_us": query_k_us, "unpack_us": unpack_k_us,
                             "xgmi_targets_bytes": 8 * (n - 1) * RK.cap, "xgmi_rows_bytes": 4 * R.pw * (n - 1) * RK.cap,
                             "exchange_targets_modelled_us": x_k, "exchange_rows_modelled_us": x_p,
                             "step_serial_us": serial_k, "step_overlapped_us": overlap_k,
                             "aggregate_queries_per_s_serial": n * Q / (serial_k * 1e-6),
                             "aggregate_queries_per_s_overlapped": n * Q / (overlap_k * 1e-6)}
                del RK
        out[str(n)] = e
        del R, t, recv, oi, oc
    out["how"] = ("rank 0 of N on this GPU (its 1/8 shard of the 100M-node table): the pack, the query over the "
                  "blocks it receives and the unpack timed with HIP events (eager, 20 launches each); the exchanges "
                  "modelled from the block bytes (nothing sent)")
    return out


def cold_pass(T, tgs, outs, ocnt, cnt_k, Q, moved_q, dev, stream, reps=8):
    """The kernel with the Infinity Cache emptied before each launch: a 1 GiB READ (no dirty lines
    left to write back during the kernel), then the launch between two events."""
    import torch

    flush = torch.ones((1 << 30) // 4, dtype=torch.int32, device=dev)
    ts = []
    for j in range(reps):
        _ = flush.sum()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        T.rt_closest(tgs[j % len(tgs)], cnt_k, outs[j % len(outs)], ocnt[j % len(ocnt)], stream=stream.cuda_stream)
        b.record(stream)
        torch.cuda.synchronize(dev)
        ts.append(a.elapsed_time(b) / 1e3)
    del flush
    t = float(np.median(ts))
    return {"kernel_ms": t * 1e3, "queries_per_s": Q / t, "achieved_GBs": moved_q * Q / t / 1e9,
            "frac": moved_q * Q / t / 1e9 / HBM_PEAK_GBS,
            "how": f"median of {reps} launches, each after a 1 GiB read that empties the 256 MiB Infinity Cache"}


def counts_pass(T, tgs, Q, dev, stream, reps=16):
    """The shard table's other call sites at the same batch size (kernel time per launch over rotated batches,
    K launches between two events): findClosestNodes(id, now, SEARCH_NODES = 14) (dht.cpp:3354), count 16 and 32
    (BASELINE config 4's sweep), and NodeCache::getCachedNodes(id, af, 14) (dht.cpp:1650) and 32."""
    import torch

    res = {}
    for name, fn, k in (("rt_k14", T.rt_closest, 14), ("rt_k16", T.rt_closest, 16), ("rt_k32", T.rt_closest, 32),
                        ("nc_k14", T.nc_closest, 14), ("nc_k32", T.nc_closest, 32)):
        out = [torch.empty((Q, k), dtype=torch.int32, device=dev) for _ in range(2)]
        cnt = [torch.empty((Q,), dtype=torch.uint8, device=dev) for _ in range(2)]
        for j in range(2):
            fn(tgs[j], k, out[j], cnt[j], stream=stream.cuda_stream)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for j in range(reps):
            fn(tgs[j % len(tgs)], k, out[j % 2], cnt[j % 2], stream=stream.cuda_stream)
        b.record(stream)
        torch.cuda.synchronize(dev)
        us = a.elapsed_time(b) / reps * 1e3
        res[name] = {"us_per_launch": us, "queries_per_s": Q / (us * 1e-6)}
    res["how"] = (f"{reps} launches of {Q} queries over rotated target batches between two HIP events (eager launches), "
                  "the bench shard's own line sets; rt = RoutingTable::findClosestNodes, nc = NodeCache::getCachedNodes")
    return res


def latency_pass(dev, nodes=170, reps=2000):
    """One Dht request's findClosestNodes through the boundary: kad_rt_closest_batch_host (what
    RoutingTableMirror::findClosestNodes calls) with 1 and 64 queries on a live-sized table (~170 nodes in the
    reference split policy, SURVEY.md §6: the reference answers one such call in ~8 us at 10k nodes).
    Beside it, the structure-faithful CPU restatement (oracle/, the port) on the same table and targets."""
    from opendht_amd import DeviceTable
    from opendht_amd import synth as S
    from opendht_amd._lib import check, lib, ptr

    ids = S.random_ids(nodes, 0x1A7)
    st = S.random_status(nodes, 0x1A8, 80, 10)
    perm, first, off = S.split_table(ids, 8)
    ids, st = np.ascontiguousarray(ids[perm]), np.ascontiguousarray(st[perm])
    tg = S.random_targets(4096, seed=0x1A9)
    res = {"nodes": nodes, "buckets": int(first.shape[0])}
    with DeviceTable(ids, st, first, off, device=dev.index or 0) as T:
        for q in (1, 64):
            if os.environ.get("KAD_LATENCY_AB"):  # synchronisation variants of the small host batch
                for mode in ("noorder", "spin", "noorder,spin"):
                    os.environ["KAD_SMALL_SYNC"] = mode
                    ts = []
                    oi, oc = np.zeros((q, 8), np.uint32), np.zeros((q,), np.uint8)
                    for r in range(reps):
                        x = np.ascontiguousarray(tg[(r * q) % (4096 - q):(r * q) % (4096 - q) + q])
                        t0 = time.perf_counter()
                        check(lib().kad_rt_closest_batch_host(T.handle, ptr(x), q, 8, ptr(oi), ptr(oc)), "host batch")
                        ts.append(time.perf_counter() - t0)
                    res[f"ab_{mode}_q{q}_us"] = float(np.median(ts)) * 1e6
                os.environ.pop("KAD_SMALL_SYNC", None)
            oi, oc = np.zeros((q, 8), np.uint32), np.zeros((q,), np.uint8)
            ts = []
            for r in range(reps):
                x = np.ascontiguousarray(tg[(r * q) % (4096 - q):(r * q) % (4096 - q) + q])
                t0 = time.perf_counter()
                check(lib().kad_rt_closest_batch_host(T.handle, ptr(x), q, 8, ptr(oi), ptr(oc)), "host batch")
                ts.append(time.perf_counter() - t0)
            res[f"gpu_call_q{q}_us"] = float(np.median(ts)) * 1e6
        # the resident query service (kad_table_serve): no launch, no stream synchronise per call
        T.serve(100_000)
        for q in (1, 64):
            oi, oc = np.zeros((q, 8), np.uint32), np.zeros((q,), np.uint8)
            ts, busy = [], []
            for r in range(reps):
                x = np.ascontiguousarray(tg[(r * q) % (4096 - q):(r * q) % (4096 - q) + q])
                t0 = time.perf_counter()
                check(lib().kad_rt_closest_batch_host(T.handle, ptr(x), q, 8, ptr(oi), ptr(oc)), "served batch")
                ts.append(time.perf_counter() - t0)
            for r in range(200):  # the device side of a request, apart from the timed calls
                x = np.ascontiguousarray(tg[(r * q) % (4096 - q):(r * q) % (4096 - q) + q])
                check(lib().kad_rt_closest_batch_host(T.handle, ptr(x), q, 8, ptr(oi), ptr(oc)), "served batch")
                busy.append(T.serve_stats()["last_busy_ns"])
            res[f"serve_q{q}_us"] = float(np.median(ts)) * 1e6
            res[f"serve_q{q}_p99_us"] = float(np.percentile(ts, 99)) * 1e6
            res[f"serve_q{q}_device_us"] = float(np.median(busy)) / 1e3
        res["serve_launches"] = int(T.serve_stats()["launches"])
        T.serve(0)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O

    F = O.FaithfulTable(ids, st, first, off)
    ts = []
    for r in range(reps):
        x = np.ascontiguousarray(tg[r % 4096:r % 4096 + 1])
        t0 = time.perf_counter()
        F.rt_closest(x, 8, nthreads=1)
        ts.append(time.perf_counter() - t0)
    F.close()
    res["cpu_port_call_us"] = float(np.median(ts)) * 1e6
    res["how"] = (f"median of {reps} synchronous calls, k=8, host buffers in and out (ctypes overhead included); "
                  "gpu: one kernel launch reading the targets from and writing the rows to mapped pinned memory; "
                  "serve: the resident query service (kad_table_serve, 100 ms idle), a request posted to and answered "
                  "from mapped pinned memory by a workgroup that stays on the GPU (device_us: from the request seen to "
                  "its rows fenced, device clock; the rest is the PCIe round trip and the host); "
                  "C-level figures without ctypes: tools/latency_serve.cpp; "
                  "cpu_port: the std::list restatement of routing_table.cpp:67-135 on one thread, same table")
    return res


def configs_pass(dev, reps=10):
    """BASELINE.json's other configs, measured beside the headline (config 3) on the same GPU: the device time per
    launch (`reps` launches over rotated target batches captured as one HIP graph) and the rows checked against the
    CPU restatement (oracle/, the checker). config 1: the reference's own CPU-runnable case, with the structure-faithful
    port timed on the same targets; config 5: the swarm model (opendht_amd/csrc/kad_swarm.hip)."""
    import torch

    from opendht_amd import DeviceTable, nc_closest_dual, rt_closest_dual
    from opendht_amd import synth as S
    from opendht_amd.swarm import Swarm

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O

    def med_ms(fn, n=reps):
        """Device time per call: n calls captured as one HIP graph (no host gaps between launches; the calls'
        line sets are built by a call before the capture), the replay timed with HIP events; the median of 3."""
        cs = torch.cuda.Stream(dev)
        fn(0, cs.cuda_stream)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cs):
            for r in range(n):
                fn(r, cs.cuda_stream)
        g.replay()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()  # the replay runs on the current stream
            g.replay()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) / n)
        del g
        return float(np.median(ts))

    def uniform(n, depth, seed):
        ids, _ = S.sort_ids(S.random_ids(n, seed))
        st = S.random_status(n, S.SEED_STATUS ^ seed)
        first, off = S.uniform_buckets(ids, depth)
        return ids, st, first, off

    res = {}
    # config 1: 10k nodes in the reference split policy, 1k targets, k = 8
    ids = S.random_ids(10_000, S.SEED_IDS)
    st = S.random_status(10_000, S.SEED_STATUS ^ S.SEED_IDS)
    perm, first, off = S.split_table(ids, 8)
    ids, st = np.ascontiguousarray(ids[perm]), np.ascontiguousarray(st[perm])
    tg = S.random_targets(1000)
    with DeviceTable(ids, st, first, off, device=dev.index or 0) as T:
        d = torch.from_numpy(tg).to(dev)
        idx, cnt = T.rt_closest(d, 8)
        ms = med_ms(lambda r, st: T.rt_closest(d, 8, idx, cnt, stream=st))
        want, wcnt = O.flat_rt_closest(ids, st, first, off, tg, 8)
        bad = int((idx.cpu().numpy().view(np.uint32) != want).any(1).sum() + (cnt.cpu().numpy() != wcnt).sum())
    F = O.FaithfulTable(ids, st, first, off)
    t0 = time.perf_counter()
    F.rt_closest(tg, 8, nthreads=1)
    port_s = time.perf_counter() - t0
    F.close()
    res["config1"] = {"what": "10,000-node table in the reference split policy, 1,000 targets, k=8",
                      "buckets": int(first.shape[0]), "gpu_batch_us": ms * 1e3, "cpu_port_1thread_us": port_s * 1e6,
                      "verified": {"rows": 1000, "mismatches": bad}}
    # config 2: 1M nodes, U(17), 64k queries, k = 8, every row checked
    ids, st, first, off = uniform(1_000_000, 17, S.SEED_IDS)
    with DeviceTable(ids, st, first, off, device=dev.index or 0, sorted=True) as T:
        tgs = [S.random_targets(1 << 16, seed=S.SEED_TARGETS + j) for j in range(4)]
        ds = [torch.from_numpy(x).to(dev) for x in tgs]
        idx, cnt = T.rt_closest(ds[0], 8)
        ms = med_ms(lambda r, st: T.rt_closest(ds[r % 4], 8, idx, cnt, stream=st))
        T.rt_closest(ds[0], 8, idx, cnt)
        want, wcnt = O.flat_rt_closest(ids, st, first, off, tgs[0], 8, nthreads=all_cores())
        bad = int((idx.cpu().numpy().view(np.uint32) != want).any(1).sum() + (cnt.cpu().numpy() != wcnt).sum())
    res["config2"] = {"what": "1,000,000-node U(17) table, 65,536 queries, k=8", "us_per_launch": ms * 1e3,
                      "queries_per_s": (1 << 16) / (ms / 1e3), "verified": {"rows": 1 << 16, "mismatches": bad}}
    # config 4: v4 and v6 tables of 1M nodes each, 1M queries with af alternating, k = 8 / 16 / 32 and NodeCache 14
    fam = [uniform(1_000_000, 17, seed) for seed in (0xC4F4, 0xC4F6)]
    Q = 1 << 20
    tgb = [S.random_targets(Q, seed=0x0D4704C4 + j) for j in range(4)]
    tg = tgb[0]
    af = (np.arange(Q) % 2).astype(np.uint8)
    c4 = {"what": "v4 + v6 tables of 1,000,000 nodes each (U(17), 80/10/10 good/expired/dubious), 1,048,576 queries, "
                  "af alternating (Dht::onGetValues asks both families, dht.cpp:3216-3217), 4 rotated target batches"}
    T4 = DeviceTable(*fam[0], device=dev.index or 0, sorted=True)
    T6 = DeviceTable(*fam[1], device=dev.index or 0, sorted=True)
    try:
        db, da = [torch.from_numpy(x).to(dev) for x in tgb], torch.from_numpy(af).to(dev)
        d = db[0]
        for k in (8, 16, 32):
            c4[f"rt_k{k}_us"] = med_ms(lambda r, st: rt_closest_dual(T4, T6, db[r % 4], da, k, stream=st)) * 1e3
        c4["nc_k14_us"] = med_ms(lambda r, st: nc_closest_dual(T4, T6, db[r % 4], da, 14, stream=st)) * 1e3
        idx, cnt = rt_closest_dual(T4, T6, d, da, 8)
        idx, cnt = idx.cpu().numpy().view(np.uint32), cnt.cpu().numpy()
        bad = 0
        for a in (0, 1):
            sel = np.flatnonzero(af[:1 << 16] == a)
            want, wcnt = O.flat_rt_closest(*fam[a][:2], *fam[a][2:], tg[sel], 8, nthreads=all_cores())
            bad += int((idx[sel] != want).any(1).sum() + (cnt[sel] != wcnt).sum())
        c4["verified"] = {"rows": 1 << 16, "mismatches": bad, "what": "the first 65,536 rows of k=8"}
    finally:
        T4.close()
        T6.close()
    res["config4"] = c4
    del fam
    # config 5: a 10M-peer swarm of shape-K tables, 1M iterative lookups to convergence (all peers online)
    ids, _ = S.sort_ids(S.random_ids(10_000_000, 0x0D470500))
    t0 = time.perf_counter()
    Wm = Swarm(ids, device=dev.index or 0)
    torch.cuda.synchronize(dev)
    build_s = time.perf_counter() - t0
    try:
        rng = np.random.default_rng(9)
        L = 1 << 20
        src = torch.from_numpy(rng.integers(0, ids.shape[0], L).astype(np.int32)).to(dev)
        tgt = torch.from_numpy(S.random_targets(L, seed=0x0D470501)).to(dev)
        # warm-up at the batch size: the timed runs take their search state (~700 bytes per lookup) from the swarm's
        # pool, as a serving loop does after its first batch; the first run (its allocations included) is `cold_ms`
        t0 = time.perf_counter()
        X = Wm.search(src, tgt)
        X.run()
        X.close()
        torch.cuda.synchronize(dev)
        cold_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        X = Wm.search(src, tgt)
        X.run()
        torch.cuda.synchronize(dev)
        run_s = time.perf_counter() - t0
        lst, q, bad_, n, hops, done, ovf = X.get(full=True)
        X.close()
        res["config5"] = {"what": "10,000,000 peers (shape-K tables in HBM, dht.cpp:867-936 policy), 1,048,576 "
                                  "lookups from random sources, alpha 4, list 14, all peers online",
                          "table_build_s": build_s, "lookups_per_s": L / run_s, "ms": run_s * 1e3,
                          "cold_ms": cold_s * 1e3,
                          "mean_hops": float(hops.mean()), "synced_frac": float((done == 1).mean()),
                          "table_GB": Wm.device_bytes() / 1e9}
        # the same lookups with 10% of the peers offline (a deterministic hash of the peer index; requests to them
        # time out and mark the node expired in the search list, search.cpp's expire path)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        X = Wm.search(src, tgt, offline_per_10k=1000)
        X.run()
        torch.cuda.synchronize(dev)
        run_s = time.perf_counter() - t0
        lst, q, bad_, n, hops, done, ovf = X.get(full=True)
        X.close()
        res["config5"]["offline_10pct"] = {"lookups_per_s": L / run_s, "ms": run_s * 1e3,
                                           "mean_hops": float(hops.mean()),
                                           "synced_frac": float((done == 1).mean())}
    finally:
        Wm.close()
    torch.cuda.empty_cache()
    return res


def host_pass(T, tgs, cnt_k, Q, dev, nb=8):
    """The PCIe-inclusive rate (targets in host memory, rows back to host memory; never the headline `value`):
    `sync_abi`: kad_rt_closest_batch_host, the synchronous host-pointer call on pageable buffers (the table's pinned
    staging, chunks pipelined over four host threads); `pipelined`: pinned host buffers, H2D + kernel + D2H of consecutive batches on two
    streams so one batch's copies overlap the other's."""
    import torch

    ht = [tgs[j % len(tgs)].cpu().pin_memory() for j in range(4)]
    from opendht_amd._lib import check, lib, ptr

    hn = ht[0].numpy().copy()  # pageable, as a caller's buffers are; result arrays reused across calls
    oi, oc = np.zeros((Q, cnt_k), np.uint32), np.zeros((Q,), np.uint8)
    ts = []
    for _ in range(6):  # the first call sets up the table's staging
        t0 = time.perf_counter()
        check(lib().kad_rt_closest_batch_host(T.handle, ptr(hn), Q, cnt_k, ptr(oi), ptr(oc)), "host batch")
        ts.append(time.perf_counter() - t0)
    sync_s = float(np.median(ts[1:]))
    ho = [torch.empty((Q, cnt_k), dtype=torch.int32).pin_memory() for _ in range(4)]
    hc = [torch.empty((Q,), dtype=torch.uint8).pin_memory() for _ in range(4)]
    dt = [torch.empty((Q, 20), dtype=torch.uint8, device=dev) for _ in range(2)]
    do = [torch.empty((Q, cnt_k), dtype=torch.int32, device=dev) for _ in range(2)]
    dc = [torch.empty((Q,), dtype=torch.uint8, device=dev) for _ in range(2)]
    ss = [torch.cuda.Stream(dev) for _ in range(2)]

    def run(n):
        for j in range(n):
            s, b = ss[j % 2], j % 2
            with torch.cuda.stream(s):
                dt[b].copy_(ht[j % 4], non_blocking=True)
                T.rt_closest(dt[b], cnt_k, do[b], dc[b], stream=s.cuda_stream)
                ho[j % 4].copy_(do[b], non_blocking=True)
                hc[j % 4].copy_(dc[b], non_blocking=True)
        torch.cuda.synchronize(dev)

    run(2)
    t0 = time.perf_counter()
    run(nb)
    pipe_s = time.perf_counter() - t0
    bytes_q = 20 + 4 * cnt_k + 1
    return {"sync_abi_queries_per_s": Q / sync_s, "pipelined_queries_per_s": nb * Q / pipe_s,
            "pcie_bytes_per_query": bytes_q, "pipelined_GBs": nb * Q * bytes_q / pipe_s / 1e9,
            "how": f"sync_abi: kad_rt_closest_batch_host over {Q} queries (pageable host buffers in and out, the "
                   f"result arrays reused across calls; "
                   f"inside, 64k-query chunks through pinned staging on two streams per host thread, four threads), "
                   f"median of 5; pipelined: {nb} batches of {Q}, pinned host buffers, H2D + "
                   "kernel + D2H per batch on two alternating streams, wall clock. Not the headline: the "
                   "boundary's device-pointer batch API is the path measured by `value`"}


def refresh_pass(T, sh, tgs, outs, ocnt, cnt_k, Q, avg_kernel_s, dev, stream, reps=5):
    """Cost of keeping every node's isGood(now) / isExpired() current on the device (node.cpp:34-40).
    kad_table_refresh_status(now) keeps the nodes' deadlines min(time + 10 min, reply_time + 120 min) sorted:
    a refresh re-derives only the nodes whose deadline `now` passed and the patched ones, and returns without
    touching the GPU while `now` is below the next deadline. The node times are those of a live table (good
    nodes heard over the last 10 minutes), so moving `now` by dt ages ~dt / 10 min of the good nodes."""
    import torch

    now = 10**15
    n = sh.ids.shape[0]
    t, rt, ex = node_times(sh.status, now)
    T.set_times(t, rt, ex)
    MIN = 60 * 10**9
    D = np.sort(np.minimum(t + 10 * MIN, rt + 120 * MIN)[ex == 0])

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        h0 = time.perf_counter()
        a.record(stream)
        fn()
        b.record(stream)
        h1 = time.perf_counter()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b), (h1 - h0) * 1e3  # GPU ms (events), host ms of the call

    first = timed(lambda: T.refresh_status(now, stream=stream.cuda_stream))  # every node, the deadline runs built
    torch.cuda.synchronize(dev)
    # `now` moving by 1 ns .. 1 us: below the next deadline, so no GPU work at all
    nf = [timed(lambda j=j: T.refresh_status(now + 1 + j, stream=stream.cuda_stream)) for j in range(reps)]
    now += 1 + reps
    ticks = {}
    for dt_ms in (1, 10, 100, 1000, 10000):  # one refresh after `now` moved by dt: the deadlines it passes
        t0 = now
        now += dt_ms * 10**6
        flips = int(np.searchsorted(D, now, "left") - np.searchsorted(D, t0, "left"))
        g_ms, h_ms = timed(lambda: T.refresh_status(now, stream=stream.cuda_stream))
        ticks[f"{dt_ms}ms"] = {"gpu_ms": g_ms, "host_call_ms": h_ms, "aged_nodes": flips}
    live, now = live_pass(T, sh, tgs, outs, ocnt, cnt_k, Q, dev, stream, now, t, rt, ex, D)
    rng = np.random.default_rng(0xF11)
    st_now = T.export_status()
    good = np.flatnonzero(st_now & 1).astype(np.uint32)
    ageing = {}
    for frac in (0.001, 0.01):  # that share of the good nodes reported last heard 10 min + 1 ns before `now`
        sel = rng.choice(good, size=int(good.shape[0] * frac), replace=False).astype(np.uint32)
        now += 10**6
        T.patch_times(sel, np.full(sel.shape[0], now - 10 * MIN - 1, np.int64), np.full(sel.shape[0], now, np.int64),
                      np.zeros(sel.shape[0], np.uint8))
        ageing[f"{frac:g}"] = timed(lambda: T.refresh_status(now, stream=stream.cuda_stream))[0]
        T.patch_times(sel, np.full(sel.shape[0], now, np.int64), np.full(sel.shape[0], now, np.int64),
                      np.zeros(sel.shape[0], np.uint8))
        T.refresh_status(now, stream=stream.cuda_stream)
        torch.cuda.synchronize(dev)
    patch = {}
    st = T.export_status()
    for frac in (0.001, 0.01, 0.1):
        m = int(n * frac)
        nodes = rng.choice(n, size=m, replace=False).astype(np.uint32)
        vals = st[nodes] ^ np.uint8(1)  # good <-> dubious
        t0 = time.perf_counter()
        T.patch_status(nodes, vals)
        patch[f"{frac:g}"] = (time.perf_counter() - t0) * 1e3
        T.patch_status(nodes, st[nodes])  # back
    no_flip_gpu = float(np.median([x[0] for x in nf]))
    no_flip_host = float(np.median([x[1] for x in nf]))
    return {"refresh_no_flip_ms": no_flip_gpu,
            "refresh_no_flip_host_call_ms": no_flip_host,
            "refresh_first_ms": first[0],
            "refresh_tick_ms": ticks,
            "refresh_ageing_ms": ageing,
            "patch_status_ms": patch,
            "nodes": int(n),
            "live": live,
            "how": "refresh_no_flip: kad_table_refresh_status(now) with `now` moved by 1 ns .. 5 ns (below the next "
                   "isGood deadline: the call returns without GPU work), median of 5: GPU time between HIP events and "
                   "the host time of the call; refresh_first: the first refresh after set_times (every node, the "
                   "deadline runs sorted); refresh_tick: one refresh after `now` moved by dt, aged_nodes = the good "
                   "nodes whose deadline it passes (live-table times: good nodes heard over the last 10 min); "
                   "refresh_ageing: patch_times of that share of the good nodes as last heard 10 min + 1 ns ago, "
                   "then the refresh (GPU ms); patch_status: kad_table_patch_status of a random changed-node list of "
                   "that share of the nodes (host list, synchronous, wall clock incl. the H2D copy); "
                   "live: see its own `how`"}


def live_pass(T, sh, tgs, outs, ocnt, cnt_k, Q, dev, stream, now, t, rt, ex, D, K=1000, W=50, vrows=65536):
    """The query rate with `now` following the clock, as a live node calls the table (routing_table.cpp:77 and
    node.cpp:34-40 evaluate isGood(now) on every call): each step is kad_table_refresh_status(now) with `now` =
    the start time + the wall-clock time elapsed since, then one batch of Q queries on the same stream (a
    distinct batch per step). The node times are a live table's (good nodes heard over the last 10 minutes:
    a deadline passes every ~60 us on a 1/8 shard), so most refreshes return at once and the others re-derive
    the nodes whose deadline passed (the small refresh: one launch that also rebuilds the lines). Eager issue
    through direct C-ABI calls (ctypes, no per-step events); the same loop without the refresh gives the share
    the refreshes take. The last step's first `vrows` rows are checked against the CPU restatement at that
    step's `now`."""
    import ctypes as C

    import torch

    from opendht_amd._lib import lib

    MIN = 60 * 10**9
    NB = len(tgs)
    L = lib()
    h, s = T._h, C.c_void_p(stream.cuda_stream)
    rt_fn, rf_fn = L.kad_rt_closest_batch, L.kad_table_refresh_status
    P = [(C.c_void_p(tgs[j].data_ptr()), C.c_void_p(outs[j].data_ptr()), C.c_void_p(ocnt[j].data_ptr()))
         for j in range(NB)]

    def loop(refresh, start):
        nows = []
        t0 = time.perf_counter()
        for j in range(K):
            if refresh:
                nw = start + int((time.perf_counter() - t0) * 1e9)
                nows.append(nw)
                if rf_fn(h, C.c_int64(nw), s):
                    raise RuntimeError("kad_table_refresh_status failed")
            tp, op, cp = P[j % NB]
            if rt_fn(h, tp, Q, cnt_k, op, cp, s):
                raise RuntimeError("kad_rt_closest_batch failed")
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, nows

    for j in range(W):  # warm-up: the same loop, untimed, `now` moving 30 us per step
        now += 30_000
        rf_fn(h, C.c_int64(now), s)
        tp, op, cp = P[j % NB]
        rt_fn(h, tp, Q, cnt_k, op, cp, s)
    torch.cuda.synchronize(dev)
    wall0, _ = loop(False, now)
    start = now + 1
    wall, nows = loop(True, start)
    passed = np.diff(np.searchsorted(D, np.array([start] + nows), "left"))
    # the last step at its `now`: isGood / isExpired from the host copies of the times
    st = (((ex == 0) & (rt >= nows[-1] - 120 * MIN) & (t >= nows[-1] - 10 * MIN)).astype(np.uint8) |
          (ex << 1)).astype(np.uint8)
    last = (K - 1) % NB
    vr = min(Q, vrows)
    bad = verify_rows(sh.ids, st, sh.first, sh.off, sh.index_base, tgs[last][:vr].cpu().numpy(),
                      outs[last][:vr].cpu().numpy(), ocnt[last][:vr].cpu().numpy(), cnt_k)
    # single refreshes passing k deadlines, as in the loop: queued behind a query batch, so the device runs the
    # refresh as soon as the batch ends (event a) and b - a is its device time (k = 0: the events' own floor);
    # host_us: the call's host time
    ticks = {}
    now = nows[-1]
    for k in (0, 1, 4, 16, 64, 100):
        i0 = int(np.searchsorted(D, now, "left"))
        nxt = now + 1 if k == 0 else int(D[min(D.shape[0] - 1, i0 + k - 1)]) + 1
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        tp, op, cp = P[k % NB]
        rt_fn(h, tp, Q, cnt_k, op, cp, s)
        a.record(stream)
        h0 = time.perf_counter()
        rf_fn(h, C.c_int64(nxt), s)
        h1 = time.perf_counter()
        b.record(stream)
        torch.cuda.synchronize(dev)
        ticks[str(k)] = {"gpu_us": a.elapsed_time(b) * 1e3, "host_us": (h1 - h0) * 1e6,
                         "passed": int(np.searchsorted(D, nxt, "left") - i0)}
        now = nxt
    live = {"queries_per_s": Q * K / wall,
            "ms_per_step": wall / K * 1e3,
            "ms_per_step_without_refresh": wall0 / K * 1e3,
            "refresh_share": max(0.0, 1.0 - wall0 / wall),
            "steps": K,
            "now_advanced_ms": (nows[-1] - start) / 1e6,
            "deadlines_passed": int(passed.sum()),
            "refreshes_with_gpu_work": int((passed > 0).sum()),
            "single_refresh_us": ticks,
            "verified": {"rows": vr, "mismatches": bad,
                         "what": "the first rows of the last step against the CPU restatement at that step's `now`"},
            "how": "K steps of refresh_status(now = start + elapsed wall time) + one Q-query batch on one stream, "
                   "eager through direct C-ABI calls; queries_per_s = K*Q / wall; refresh_share = 1 - (the same loop "
                   "without the refresh) / wall; single_refresh_us: one refresh passing k deadlines queued behind a query "
                   "batch, its device time between an event after the batch and one after the refresh (k = 0: the "
                   "events' floor, no GPU work), and the host time of the call"}
    return live, now + 1


# ---------------------------------------------------------------------------------------------
# north-star variant: halo-free shards, replicated batch, all-gather + device merge
# ---------------------------------------------------------------------------------------------
def graph_steps(step, K, W, dev, dist, use_graph=True):
    """W untimed warm-up steps, then exactly K steps (one HIP graph of K steps unless use_graph is False)
    between a barrier + synchronize on both sides. step(j) issues step j on the current stream.
    Returns (max wall over ranks, the kernels' average ms per step from HIP events, launch kind)."""
    import torch

    stream = torch.cuda.current_stream(dev)
    for j in range(W):
        step(K + j)
    torch.cuda.synchronize(dev)
    graph = None
    if use_graph:
        try:
            g = torch.cuda.CUDAGraph()
            cs = torch.cuda.Stream(dev)
            cs.wait_stream(stream)
            with torch.cuda.graph(g, stream=cs):
                for j in range(K):
                    step(j)
            stream.wait_stream(cs)
            torch.cuda.synchronize(dev)
            g.replay()  # the first replay uploads the graph
            torch.cuda.synchronize(dev)
            graph = g
        except Exception as e:
            print(f"graph capture failed ({e}); eager launches", file=sys.stderr)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if dist:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    a.record(stream)
    if graph is not None:
        graph.replay()
    else:
        for j in range(K):
            step(j)
    b.record(stream)
    torch.cuda.synchronize(dev)
    if dist:
        dist.barrier()
    wall = time.perf_counter() - t0
    return max_over_ranks(dist, wall, dev), a.elapsed_time(b) / K, ("hip graph of K steps" if graph is not None
                                                                     else "K eager steps")


def allgather_pass(args, world, rank, local, dev, dist):
    """The north-star variant: the 100M-node table in `world` halo-free shards, the same
    1M-query batch on every rank, each rank's part of every window into the send block of the query's home
    rank, one all_to_all of fixed-size blocks (each rank receives its ~Q/world home queries' rows), the device
    scatter + merge; no host read inside the K steps (the overflow word is combined and read after them)."""
    import torch

    from opendht_amd.global_shard import GlobalShard, build_plain_shard, global_good_prefix, home_range
    from opendht_amd.sharded import build_shard, config3_spec
    from opendht_amd.synth import bucket_firsts

    if world & (world - 1) or world > 8:
        return {"skipped": "world size must be a power of two <= 8"}
    spec = config3_spec(world)  # the 100M-node U(24) table in `world` shards
    t0 = time.perf_counter()
    ids, st, off, lo, hi, base, good = build_plain_shard(spec, rank)
    gp = global_good_prefix(good, device=dev if world > 1 else None)
    G = GlobalShard(ids, st, off, lo, hi, spec.depth, base, gp, device=local)
    n_local = ids.shape[0]
    Q, K, cnt_k = args.queries, max(4, min(args.steps, 20)), args.count
    NB = K + 2
    tgs = device_targets(NB, Q, 0, 0, 0x0D470002, dev)  # the same global batches on every rank
    out_idx = torch.empty((Q, cnt_k), dtype=torch.int32, device=dev)  # (home rows first at N > 1)
    out_cnt = torch.empty((Q,), dtype=torch.uint8, device=dev)
    setup = time.perf_counter() - t0
    vrows = min(Q, args.verify_rows)
    res = {"unit": "queries/s", "n_gpus": world, "steps": K, "scaling": "strong", "setup_s": setup}
    if world == 1:
        # one rank holds the whole table: the query is the plain batch (nothing to exchange)
        t_max, kern_ms, how = graph_steps(lambda j: G.table.rt_closest(tgs[j % NB], cnt_k, out_idx, out_cnt), K, 2,
                                          dev, None)
        first = bucket_firsts(spec.depth, lo, hi)
        vt = tgs[(K - 1) % NB][:vrows].cpu().numpy()
        bad = verify_rows(ids, st, first, off, 0, vt, out_idx[:vrows].cpu().numpy(), out_cnt[:vrows].cpu().numpy(),
                          cnt_k)
        res.update({"value": Q * K / t_max, "ms_per_step": t_max / K * 1e3, "avg_kernel_ms": kern_ms, "launch": how,
                    "workload": f"100M-node U(24) table whole on one GPU ({n_local} nodes), {Q} queries per step "
                                f"(a distinct batch per step), k={cnt_k}: the plain batch",
                    "verified": {"rows": vrows, "mismatches": bad}})
        # what each rank runs at N > 1 minus the collective: shard kernel + kad_rt_home_finish, as a graph
        ex = G.exchange(Q, cnt_k, 1)
        t_sh, kern_sh, how_sh = graph_steps(lambda j: G.step(tgs[j % NB], ex, out_idx, out_cnt), K, 2, dev, None)
        ovf = ex.overflowed()
        bad_sh = verify_rows(ids, st, first, off, 0, vt, out_idx[:vrows].cpu().numpy(),
                             out_cnt[:vrows].cpu().numpy(), cnt_k)
        res["shard_kernel_path"] = {"ms_per_step": t_sh / K * 1e3, "avg_kernel_ms": kern_sh, "launch": how_sh,
                                    "overflow": ovf, "verified": {"rows": vrows, "mismatches": bad_sh},
                                    "how": "N = 1 through kad_rt_shard_batch_home + kad_rt_home_finish (device-only "
                                           "step) instead of the plain batch"}
        # the exchange each rank would receive at N = 2, 4, 8 for this Q and count (layouts only, nothing sent)
        res["exchange_model"] = exchange_model(Q, cnt_k, dev)
        # rank 0's device work at N = 8, timed here on its shard of the same table: the shard kernel over the
        # replicated batch into 8 home blocks, and the finish over 8 blocks of its rows (copies of its own block
        # to itself: the other ranks' blocks have the same shape); with the modelled all_to_all, a step's time and
        # the aggregate rate N = 8 ranks would reach on this replicated batch
        try:
            res["n8_step_model"] = n8_step_model(ids, st, off, gp if world == 1 else None, spec, tgs, Q, cnt_k, K, NB,
                                                 dev, res["exchange_model"]["8"]["home_modelled_us"])
        except Exception as e:  # a model, never the line's failure
            res["n8_step_model"] = {"error": f"{type(e).__name__}: {e}"}
        if not args.no_rccl1:
            G.close()
            res["rccl_world1"] = rccl_world1_child(args)
    else:
        ex = G.exchange(Q, cnt_k, world)
        lo, hi = home_range(Q, world, rank)
        oi, oc = out_idx[:hi - lo], out_cnt[:hi - lo]
        for _ in range(4):  # capacities: grow until a step fits (the counters combined over the ranks)
            G.step(tgs[K], ex, oi, oc, rank=rank)
            if not ex.overflowed():
                break
            ex = G._ex[(Q, cnt_k, world, True, world > 1)] = ex.grown()
        for _ in range(3):
            t_max, kern_ms, how = graph_steps(lambda j: G.step(tgs[j % NB], ex, oi, oc, rank=rank), K, 1, dev, dist,
                                              use_graph=False)
            if not ex.overflowed():
                break
            ex = G._ex[(Q, cnt_k, world, True, world > 1)] = ex.grown()
        else:
            raise RuntimeError("exchange buffers kept overflowing")
        try:
            pipe, pi, pc = north_star_pipelined(G, ex, tgs, Q, cnt_k, K, NB, dev, dist, world, rank)
        except Exception as e:
            pipe, pi = {"error": f"{type(e).__name__}: {e}"}, None
        nat, nrows = None, {}
        if dist.get_backend() == "nccl":  # the native executor (its own communicator; the id over this group)
            try:
                from opendht_amd.comm import Comm

                with Comm(local, world, rank) as comm:
                    nat, nrows = north_star_native(G, ex, tgs, Q, cnt_k, K, NB, dev, dist, world, rank, comm)
            except Exception as e:
                nat = {"error": f"{type(e).__name__}: {e}"}
        # verification: this rank's home rows (queries [lo, hi)) among the first vrows whose targets this rank
        # owns, against the restatement on this rank's shard WITH its exact halo (every owned window lies inside)
        G.close()
        del ids, st
        vh = min(hi, vrows) - lo if lo < vrows else 0
        vt = tgs[(K - 1) % NB][lo:lo + max(vh, 0)].cpu().numpy()
        own = (vt[:, 0].astype(np.int64) >> (8 - spec.shard_bits)) == rank
        sh = build_shard(spec, rank)
        bad = verify_rows(sh.ids, sh.status, sh.first, sh.off, sh.index_base, vt[own],
                          oi[:vt.shape[0]].cpu().numpy()[own], oc[:vt.shape[0]].cpu().numpy()[own], cnt_k)
        if pi is not None:
            pbad = verify_rows(sh.ids, sh.status, sh.first, sh.off, sh.index_base, vt[own],
                               pi[:vt.shape[0]].cpu().numpy()[own], pc[:vt.shape[0]].cpu().numpy()[own], cnt_k)
            pipe["verified"] = {"rows": sum_over_ranks(dist, int(own.sum()), dev),
                                "mismatches": sum_over_ranks(dist, pbad, dev)}
        res["pipelined"] = pipe
        for m, (ni, nc) in nrows.items():
            nb = verify_rows(sh.ids, sh.status, sh.first, sh.off, sh.index_base, vt[own],
                             ni[:vt.shape[0]].cpu().numpy()[own], nc[:vt.shape[0]].cpu().numpy()[own], cnt_k)
            nat[m]["verified"] = {"rows": sum_over_ranks(dist, int(own.sum()), dev),
                                  "mismatches": sum_over_ranks(dist, nb, dev)}
        if nat is not None:
            res["native"] = nat
        res.update({"value": Q * K / t_max, "ms_per_step": t_max / K * 1e3, "avg_step_ms_events": kern_ms,
                    "launch": how,
                    "workload": f"100M-node U(24) table, 1/{world} per GPU without halo ({n_local} nodes on rank 0), "
                                f"{Q} global queries per step (a distinct batch per step, replicated on every rank), "
                                f"k={cnt_k}; kad_rt_shard_batch_home into `world` fixed-size blocks (one per home "
                                "rank), RCCL all_to_all_single of the blocks, kad_rt_home_finish (scatter + merge of "
                                "the rank's home queries on the device)",
                    "gathered_bytes_per_step": ex.gathered_bytes,
                    "xgmi_bytes_per_step": ex.xgmi_bytes,
                    "row_cap": ex.row_cap, "part_cap": ex.part_cap,
                    "verified": {"rows": sum_over_ranks(dist, int(own.sum()), dev),
                                 "mismatches": sum_over_ranks(dist, bad, dev)}})
        return res
    G.close()
    return res


def north_star_pipelined(G, ex, tgs, Q, cnt_k, K, NB, dev, dist, world, rank):
    """The north-star step over K consecutive batches through GlobalShard.run_pipelined (three exchange buffer sets
    with ex's grown capacities; batch i+1's all_to_all under batch i's finish and batch i+2's shard kernel): eager
    and as one HIP graph of the K batches (issue_timed; RCCL only), the sticky overflow words of the three sets
    combined after. Returns (the object, this rank's home rows of the last batch)."""
    import torch

    from opendht_amd.global_shard import home_range

    lo, hi = home_range(Q, world, rank)
    exs = G.pipeline(Q, cnt_k, world, like=ex)
    outs = [(torch.empty((hi - lo, cnt_k), dtype=torch.int32, device=dev),
             torch.empty((hi - lo,), dtype=torch.uint8, device=dev)) for _ in range(NB)]
    G.run_pipelined([tgs[j % NB] for j in range(3)], exs, [outs[j % NB] for j in range(3)], None, rank)
    torch.cuda.synchronize(dev)
    over0 = any(e.overflowed() for e in exs)
    tm = issue_timed(lambda: G.run_pipelined([tgs[j % NB] for j in range(K)], exs, [outs[j % NB] for j in range(K)],
                                             None, rank), K, dev, dist, graph_ok=False)
    over = any(e.overflowed() for e in exs)
    oi, oc = outs[(K - 1) % NB]
    best = "graph" if "graph" in tm else "eager"
    res = {"value": Q * K / tm[best][0], "ms_per_step": tm[best][0] / K * 1e3, "launch": best,
           "eager_ms_per_step": tm["eager"][0] / K * 1e3, "eager_host_issue_ms_per_step": tm["eager"][1] / K * 1e3,
           "overflow": over or over0,
           "how": "GlobalShard.run_pipelined: " + G.run_pipelined.__doc__.split("\n\n")[0].replace("\n", " ")}
    if "graph_error" in tm:
        res["graph_error"] = tm["graph_error"]
    return res, oi, oc


def north_star_native(G, ex, tgs, Q, cnt_k, K, NB, dev, dist, world, rank, comm):
    """The north-star step over K batches through the native executor (opendht_amd.comm.shard_run: kad_shard_run over
    the engine's own RCCL communicator, one C call per run): one exchange set (serial) and three (pipelined), with ex's
    grown capacities. Returns ({mode: object}, {mode: this rank's home rows of the last batch})."""
    import torch

    from opendht_amd.comm import shard_run
    from opendht_amd.global_shard import home_range

    lo, hi = home_range(Q, world, rank)
    res, rows = {}, {}
    for name, n in (("serial", 1), ("pipelined", 3)):
        exs = G.pipeline(Q, cnt_k, world, like=ex)[:n]
        outs = [(torch.empty((hi - lo, cnt_k), dtype=torch.int32, device=dev),
                 torch.empty((hi - lo,), dtype=torch.uint8, device=dev)) for _ in range(NB)]
        shard_run(G, comm, [tgs[j % NB] for j in range(3)], exs, [outs[j % NB] for j in range(3)])
        torch.cuda.synchronize(dev)
        over0 = exs[0].overflowed()
        tm = issue_timed(lambda: shard_run(G, comm, [tgs[j % NB] for j in range(K)], exs,
                                           [outs[j % NB] for j in range(K)]), K, dev, dist, graph_ok=False)
        t_max, host = tm["eager"]
        res[name] = {"value": Q * K / t_max, "ms_per_step": t_max / K * 1e3, "host_issue_ms_per_step": host / K * 1e3,
                     "overflow": over0 or exs[0].overflowed()}
        rows[name] = outs[(K - 1) % NB]
    res["how"] = north_star_native.__doc__.split("\n\n")[0].replace("\n", " ")
    return res, rows


def home0_recv(G0, ex, tg, Q, dev):
    """The blocks rank 0 receives at N = 8, in shape: 8 blocks addressed to home 0, block c holding this shard's rows
    of the home-0 queries i = c (mod 8) (their targets moved into this shard, every other target beyond its reach), so
    that each home query is answered in exactly one block with the row volume of a uniform batch."""
    import torch

    ctr = ex.send.view(8, ex.block)[:, ex.ctr_off:ex.ctr_off + 10 * 32]
    sel = torch.arange(Q, device=dev) % 8
    blocks = []
    for c in range(8):
        t = tg.clone()
        t[:, 0] = torch.where(sel == c, t[:, 0] & 0x1F, t[:, 0] | 0x80)
        ctr.zero_()
        G0.home_block(t, ex, zeroed=True)
        blocks.append(ex.send[:ex.block].clone())
    recv = torch.cat(blocks)
    if bool((recv.view(8, ex.block)[:, ex.ctr_off + 9 * 32] != 0).any()):  # a block's sticky overflow word
        raise RuntimeError("home-0 blocks overflowed their capacities")
    return recv


def n8_step_model(ids, st, off, gp, spec, tgs, Q, cnt_k, K, NB, dev, xchg_us):
    """Rank 0's kernels at N = 8 (see allgather_pass), HIP events around K eager launches each."""
    import torch

    from opendht_amd.global_shard import GlobalShard

    B = off.shape[0] - 1
    hi = B // 8
    n0 = int(off[hi])
    G0 = GlobalShard(ids[:n0], st[:n0], off[:hi + 1], 0, hi, spec.depth, 0, gp, device=dev.index or 0)
    try:
        import ctypes as C

        stream = torch.cuda.current_stream(dev)
        s = C.c_void_p(stream.cuda_stream)
        out = {"shard_nodes": n0}
        for k in sorted({cnt_k, 32}):
            ex = G0.exchange(Q, k, 8, True, True)
            ctr = ex.send.view(8, ex.block)[:, ex.ctr_off:ex.ctr_off + 10 * 32]
            for j in range(2):
                ctr.zero_()
                G0.home_block(tgs[j % NB], ex, zeroed=True)
            # per launch, the counters zeroed between launches outside the timed interval (the step's own finish
            # zeroes them: kad_rt_home_finish_reset)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(K)]
            for j in range(K):
                ctr.zero_()
                ev[j][0].record(stream)
                G0.home_block(tgs[j % NB], ex, zeroed=True)
                ev[j][1].record(stream)
            torch.cuda.synchronize(dev)
            shard_us = float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3
            over = ex.overflowed(combine=False)
            G0.home_block(tgs[0], ex, zeroed=False)  # (the old form with its zeroing launch, for comparison)
            torch.cuda.synchronize(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for j in range(K):
                G0.home_block(tgs[j % NB], ex, zeroed=False)
            b.record(stream)
            torch.cuda.synchronize(dev)
            shard_zeroing_us = a.elapsed_time(b) / K * 1e3
            ex.recv = home0_recv(G0, ex, tgs[0], Q, dev)
            hi_q = -(-(-(-Q // 256)) // 8) * 256
            oi = torch.empty((min(hi_q, Q), k), dtype=torch.int32, device=dev)
            oc = torch.empty((min(hi_q, Q),), dtype=torch.uint8, device=dev)
            ex.home_finish(0, oi, oc, s, reset=True)
            torch.cuda.synchronize(dev)
            a.record(stream)
            for j in range(K):
                ex.home_finish(0, oi, oc, s, reset=True)
            b.record(stream)
            torch.cuda.synchronize(dev)
            fin_us = a.elapsed_time(b) / K * 1e3
            xm = exchange_model(Q, k, dev)["8"]["home_modelled_us"] if k != cnt_k else xchg_us
            step_us = shard_us + xm + fin_us
            out[f"k{k}"] = {"shard_kernel_us": shard_us, "shard_kernel_with_zeroing_launch_us": shard_zeroing_us,
                            "overflow": over, "finish_us": fin_us, "exchange_modelled_us": xm,
                            "step_modelled_us": step_us, "aggregate_queries_per_s_modelled": Q / (step_us * 1e-6)}
            del ex, oi, oc
        # the reach-0 floor: the same kernel on a batch none of whose targets this shard can reach (reading and
        # testing the batch is all it does)
        ex = G0.exchange(Q, cnt_k, 8, True, True)
        far = [t.clone() for t in tgs[:4]]
        for t in far:
            t[:, 0] = t[:, 0] | 0x80  # buckets in the upper half of the table: beyond rank 0's reach
        ctr = ex.send.view(8, ex.block)[:, ex.ctr_off:ex.ctr_off + 10 * 32]
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(K)]
        for j in range(K):
            ctr.zero_()
            ev[j][0].record(stream)
            G0.home_block(far[j % 4], ex, zeroed=True)
            ev[j][1].record(stream)
        torch.cuda.synchronize(dev)
        out["reach0_shard_kernel_us"] = float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3
        top = out[f"k{cnt_k}"]
        out.update({"shard_kernel_us": top["shard_kernel_us"], "finish_us": top["finish_us"],
                    "exchange_modelled_us": xchg_us, "step_modelled_us": top["step_modelled_us"],
                    "aggregate_queries_per_s_modelled": top["aggregate_queries_per_s_modelled"]})
        out["how"] = ("rank 0 of 8 (global buckets [0, B/8), no halo) on this GPU: kad_rt_shard_step_home over the "
                      "whole replicated batch into 8 home blocks (HIP events around each launch, median; the "
                      "counters zeroed between launches outside them, as kad_rt_home_finish_reset leaves them), "
                      "kad_rt_home_finish_reset over 8 blocks addressed to home 0 (block c: this shard's rows of the "
                      "home-0 queries i = c mod 8, so that every home query is answered once, as when 8 shards "
                      "answer it); + "
                      "the modelled all_to_all at N = 8. The eight ranks answer the one batch together, so the "
                      "aggregate is Q / step")
        return out
    finally:
        G0.close()


def exchange_model(Q, count, dev, link_gbs=64.0):
    """The home exchange's per-rank bytes at N = 2, 4, 8 for a Q-query step (the default layouts, nothing sent),
    and a modelled all_to_all time: each rank receives world - 1 blocks, each over its own xGMI link, at
    link_gbs GB/s per link (a conservative one-direction rate for one of the 7 links of an MI355X), plus ~10 us of
    collective latency. The all-gather layout's bytes beside it."""
    from opendht_amd.global_shard import Exchange

    out = {"link_GBps_assumed": link_gbs, "latency_us_assumed": 10.0}
    for n in (2, 4, 8):
        h = Exchange(Q, count, n, dev, home=True)
        g = Exchange(Q, count, n, dev, home=False)
        out[str(n)] = {"home_gathered_bytes": h.gathered_bytes, "home_xgmi_bytes": h.xgmi_bytes,
                       "home_modelled_us": 10.0 + 4 * h.block / (link_gbs * 1e3),
                       "allgather_gathered_bytes": g.gathered_bytes,
                       "allgather_modelled_us": 10.0 + 4 * g.block / (link_gbs * 1e3)}
        del h, g
    return out


def allgather_child(args, world, rank, local, dist) -> dict:
    """The north-star variant at N > 1 in child processes (rank_child)."""
    return rank_child(args, world, rank, local, dist, "allgather-child")


def owner_child(args, world, rank, local, dist) -> dict:
    """The owner-routed serving step at N > 1 in child processes (rank_child, main_owner_child): its data path runs on
    an RCCL group, and a failing or hanging RCCL collective can cost only the `owner_routed` object."""
    return rank_child(args, world, rank, local, dist, "owner-child")


def rank_child(args, world, rank, local, dist, mode) -> dict:
    """A part of the line measured at N > 1 in child processes (one per rank, the same GPU), so that a failing or
    hanging RCCL collective can cost only that object, never the headline line: each rank starts its child with a
    shared fresh port and waits at most --ag-timeout seconds."""
    import tempfile

    port = [0]
    if rank == 0:
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port[0] = so.getsockname()[1]
    dist.broadcast_object_list(port, src=0)
    out = os.path.join(tempfile.gettempdir(), f"kadgpu_{mode}_{port[0]}_{rank}.json")
    env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(local), WORLD_SIZE=str(world),
               LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port[0]))
    argv = [sys.executable, "-u", os.path.abspath(__file__), "--gpus", str(world), "--mode", mode,
            "--ag-out", out, "--queries", str(args.queries), "--steps", str(args.steps), "--warmup", str(args.warmup),
            "--count", str(args.count), "--verify-rows", str(args.verify_rows)]
    p = subprocess.Popen(argv, env=env, stdout=sys.stderr)  # the child's output never reaches the JSON line
    try:
        rc = p.wait(timeout=args.ag_timeout)
    except subprocess.TimeoutExpired:
        p.kill()
        p.wait()
        return {"error": f"rank {rank}: the {mode} process was killed after {args.ag_timeout:.0f} s"}
    try:
        with open(out) as f:
            res = json.load(f)
        os.unlink(out)
    except (OSError, ValueError):
        res = {"error": f"rank {rank}: the {mode} process exited with {rc} and no result"}
    return res


def main_owner_child(args):
    """owner_routed_pass at N > 1 (owner_child): the default group is gloo (barriers, max over ranks, the verification
    gather), the data path's all_to_alls run on a second group of data_backend() — RCCL over xGMI on the driver's
    node, one GPU per rank."""
    from datetime import timedelta

    import torch
    import torch.distributed as dist

    from opendht_amd import DeviceTable
    from opendht_amd.sharded import build_shard, config3_spec

    world, rank, local = dist_env()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist.init_process_group("gloo", timeout=timedelta(seconds=600))
    res = {}
    try:
        be = data_backend(world, dev)
        group = dist.new_group(backend=be, timeout=timedelta(seconds=120)) if be == "nccl" else None
        spec = config3_spec()
        sh = build_shard(spec, rank)
        T = DeviceTable(sh.ids, sh.status, sh.first, sh.off, device=local, index_base=sh.index_base, sorted=True)
        comm = None
        if be == "nccl":
            from opendht_amd.comm import Comm

            comm = Comm(local, world, rank)  # the native executor's communicator (id over the gloo default group)
        try:
            res = owner_routed_pass(T, sh, spec, args.queries, args.count, args.steps, args.warmup, dev, dist, world,
                                    rank, group=group, comm=comm)
        finally:
            T.close()
            if comm is not None:
                comm.close()
    except Exception as e:
        res = {"error": f"rank {rank}: {type(e).__name__}: {e}"}
    with open(args.ag_out, "w") as f:
        json.dump(res, f)
    try:
        dist.destroy_process_group()
    except Exception:
        pass
    return 0 if "error" not in res else 1


def rccl_world1_child(args) -> dict:
    """The north-star step through a real one-rank RCCL group (rccl1_pass), in a child process with a timeout so
    that a failing RCCL initialisation costs only this object."""
    import tempfile

    out = os.path.join(tempfile.gettempdir(), f"kadgpu_rccl1_{os.getpid()}.json")
    argv = [sys.executable, "-u", os.path.abspath(__file__), "--mode", "rccl1-child", "--ag-out", out, "--queries",
            str(args.queries), "--steps", str(args.steps), "--verify-rows", str(args.verify_rows)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.Popen(argv, env=env, stdout=sys.stderr)
    try:
        rc = p.wait(timeout=args.ag_timeout)
    except subprocess.TimeoutExpired:
        p.kill()
        p.wait()
        return {"error": f"the one-rank RCCL child was killed after {args.ag_timeout:.0f} s"}
    try:
        with open(out) as f:
            res = json.load(f)
        os.unlink(out)
    except (OSError, ValueError):
        res = {"error": f"the one-rank RCCL child exited with {rc} and no result"}
    return res


def rccl1_pass(args) -> dict:
    """One rank, one real RCCL ("nccl") process group on this GPU: the north-star step with its collective forced
    on (kad_rt_shard_batch_home, all_to_all_single of the send block through RCCL, kad_rt_home_finish) beside the
    same step without it, on config 3's rank-0 shard as a table of its own (2^21 U(24) buckets, 12.5M nodes: the
    per-GPU table size, targets in its range). HIP events around K eager steps each, and around the collective
    alone; the last step's rows checked against the CPU restatement."""
    import ctypes as C
    from datetime import timedelta

    import torch
    import torch.distributed as dist

    from opendht_amd.global_shard import GlobalShard, build_plain_shard, exchange_into
    from opendht_amd.sharded import config3_spec
    from opendht_amd.synth import bucket_firsts

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev,
                            timeout=timedelta(seconds=60))
    try:
        spec = config3_spec(8)
        ids, st, off, lo, hi, base, good = build_plain_shard(spec, 0)
        gp = np.concatenate([[0], np.cumsum(good.astype(np.int64))])
        G = GlobalShard(ids, st, off, 0, hi, spec.depth, 0, gp, device=0)
        Q, K, cnt_k = args.queries, max(4, min(args.steps, 20)), 8
        NB = K + 2
        tgs = device_targets(NB, Q, spec.shard_bits, 0, 0x0D470005, dev)
        oi = torch.empty((Q, cnt_k), dtype=torch.int32, device=dev)
        oc = torch.empty((Q,), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        res = {"workload": f"config 3's rank-0 shard as a table of its own ({ids.shape[0]} nodes, {hi} U(24) buckets), "
                           f"{Q} queries per step, k={cnt_k}, one-rank RCCL group on this GPU",
               "backend": dist.get_backend()}
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for coll in (False, True):
            ex = G.exchange(Q, cnt_k, 1, True, coll)
            for _ in range(4):
                G.step(tgs[K], ex, oi, oc, rank=0)
                if not ex.overflowed():
                    break
                ex = G._ex[(Q, cnt_k, 1, True, coll)] = ex.grown()
            torch.cuda.synchronize(dev)
            a.record(stream)
            for j in range(K):
                G.step(tgs[j % NB], ex, oi, oc, rank=0)
            b.record(stream)
            torch.cuda.synchronize(dev)
            key = "rccl" if coll else "no_collective"
            res[f"step_us_{key}"] = a.elapsed_time(b) / K * 1e3
            res[f"overflow_{key}"] = ex.overflowed()
            vrows = min(Q, args.verify_rows)
            first = bucket_firsts(spec.depth, 0, hi)
            res[f"verified_{key}"] = {"rows": vrows, "mismatches": verify_rows(
                ids, st, first, off, 0, tgs[(K - 1) % NB][:vrows].cpu().numpy(), oi[:vrows].cpu().numpy(),
                oc[:vrows].cpu().numpy(), cnt_k)}
            if coll:
                res["block_bytes"] = 4 * ex.block
                torch.cuda.synchronize(dev)
                a.record(stream)
                for j in range(K):
                    exchange_into(ex.recv, ex.send)
                b.record(stream)
                torch.cuda.synchronize(dev)
                res["all_to_all_us"] = a.elapsed_time(b) / K * 1e3
                # the same K batches pipelined (the all_to_all on a comm stream under the next shard kernel)
                try:
                    pipe, pi, pc = north_star_pipelined(G, ex, tgs, Q, cnt_k, K, NB, dev, dist, 1, 0)
                    pipe["step_us"] = pipe.pop("ms_per_step") * 1e3
                    pipe["verified"] = {"rows": vrows, "mismatches": verify_rows(
                        ids, st, first, off, 0, tgs[(K - 1) % NB][:vrows].cpu().numpy(), pi[:vrows].cpu().numpy(),
                        pc[:vrows].cpu().numpy(), cnt_k)}
                    res["pipelined"] = pipe
                except Exception as e:
                    res["pipelined"] = {"error": f"{type(e).__name__}: {e}"}
                try:
                    from opendht_amd.comm import Comm

                    with Comm(0, 1, 0) as comm:
                        nat, nrows = north_star_native(G, ex, tgs, Q, cnt_k, K, NB, dev, dist, 1, 0, comm)
                        for m, (ni, nc) in nrows.items():
                            nat[m]["verified"] = {"rows": vrows, "mismatches": verify_rows(
                                ids, st, first, off, 0, tgs[(K - 1) % NB][:vrows].cpu().numpy(),
                                ni[:vrows].cpu().numpy(), nc[:vrows].cpu().numpy(), cnt_k)}
                    res["native"] = nat
                except Exception as e:
                    res["native"] = {"error": f"{type(e).__name__}: {e}"}
        G.close()
        del ids, st
        # owner routing through the one-rank RCCL group: config 3's rank-0 shard with its halo,
        # the targets (all owned by shard 0) through kad_route_pack, the RCCL all_to_all of the target blocks, the
        # packed query, the RCCL all_to_all of the packed rows, the unpack; then the same batches pipelined
        from opendht_amd import DeviceTable
        from opendht_amd.sharded import build_shard

        sh = build_shard(spec, 0)
        T = DeviceTable(sh.ids, sh.status, sh.first, sh.off, device=0, index_base=sh.index_base, sorted=True)
        from opendht_amd.comm import Comm

        comm = Comm(0, 1, 0)
        try:
            res["owner_routed"] = owner_routed_pass(T, sh, spec, Q, cnt_k, K, 2, dev, dist, 1, 0, group=None,
                                                    collective=True, pipelined=True, comm=comm)
        finally:
            T.close()
            comm.close()
        res["how"] = ("Exchange(world=1, collective=True): the all_to_all_single of the one send block runs through "
                      "RCCL (a device copy at world 1); the difference to step_us_no_collective is its cost")
        return res
    finally:
        dist.destroy_process_group()


def main_rccl1_child(args):
    try:
        res = rccl1_pass(args)
    except Exception as e:
        res = {"error": f"{type(e).__name__}: {e}"}
    with open(args.ag_out, "w") as f:
        json.dump(res, f)
    return 0 if "error" not in res else 1


def main_allgather_child(args):
    import torch

    world, rank, local = dist_env()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = init_dist(world, dev, rccl=True)
    try:
        ag = allgather_pass(args, world, rank, local, dev, dist)
    except Exception as e:
        ag = {"error": f"rank {rank}: {type(e).__name__}: {e}"}
    with open(args.ag_out, "w") as f:
        json.dump(ag, f)
    if dist:
        try:
            dist.destroy_process_group()
        except Exception:
            pass
    return 0 if "error" not in ag else 1


def main_allgather_line(args):
    import torch

    world, rank, local = dist_env()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = init_dist(world, dev, rccl=True)
    ag = allgather_pass(args, world, rank, local, dev, dist)
    if rank == 0:
        print(json.dumps({"metric": "k=8 closest-node queries/sec, 1M queries vs the 100M-node table split over N "
                                    "GPUs (north-star all-gather + merge variant)",
                          "value": ag.get("value"), "unit": "queries/s", "n_gpus": world,
                          "steps": ag.get("steps"), "warmup": 2, "ms_per_step": ag.get("ms_per_step"),
                          "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u64",
                          "data": "synthetic", "config": {"workload": ag.get("workload")}, "allgather": ag}),
              flush=True)
    if dist:
        dist.barrier()
        dist.destroy_process_group()


def main_plumbing(args):
    """The multi-process skeleton of main_owner on CPU ranks (gloo): the same env contract, barrier
    and max-over-ranks timing, rank 0 prints one line. Exercised by tests/test_bench_launcher.py."""
    import torch

    world, rank, _ = dist_env()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    dev = torch.device("cpu")
    dist = init_dist(world, dev)
    if dist:
        dist.barrier()
    t0 = time.perf_counter()
    x = torch.arange(1 << 16, dtype=torch.int64).sum().item()
    wall = time.perf_counter() - t0 + 1e-3 * rank
    t_max = max_over_ranks(dist, wall, dev)
    if rank == 0:
        print(json.dumps({"plumbing": True, "n_ranks": world, "t_max": t_max, "check": x,
                          "ranks_seen": world if dist is None else dist.get_world_size()}), flush=True)
    if dist:
        dist.barrier()
        dist.destroy_process_group()


def main(argv=None):
    args = parse_args(argv)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return spawn(args)
    if args.plumbing:
        return main_plumbing(args)
    if args.mode == "allgather":
        return main_allgather_line(args)
    if args.mode == "allgather-child":
        return main_allgather_child(args)
    if args.mode == "owner-child":
        return main_owner_child(args)
    if args.mode == "rccl1-child":
        return main_rccl1_child(args)
    return main_owner(args)


if __name__ == "__main__":
    sys.exit(main() or 0)
