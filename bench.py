#!/usr/bin/env python3
"""bench.py -- rotation hypotheses scored per second (BASELINE.json metric) on MI355X.

One "step" = the reference's per-pair hot loop (test_co3d.py:137-146) for ONE synthetic image pair against the SAME
N_hyp = 50 000 Haar hypotheses whatever the number of GPUs (BASELINE.json configs[1]; the metric is quoted "at 1/2/4/8
MI355X": strong scaling -- the hypothesis axis is cut into contiguous shards, rank r scores [lo_r, hi_r) with n_offset = lo_r):
    forward_3d2d(vol_tgt) + rotate + forward_3d2d + score + running max   ONE launch, ahv_verify_pair_f32
                                                                          (test_co3d.py:137-145)
    [N > 1: all-reduce(MAX) of the packed int64 keys over RCCL -- the keys of 8 steps per collective, in stream order]
    decode the keys, gather R_pred = proposals[idx], hand the keys back empty   ONE launch per 8 steps (test_co3d.py:145-146)
Inputs are resident in HBM before the timed region.  `value` = 50 000 x steps / time: the whole job's hypotheses per
second ("scaling": "strong").

A plain run sets up, pre-warms, runs `--warmup` untimed steps, times exactly `--steps` steps and prints the headline line;
`--dump-outputs DIR` then also writes what the last timed step handed its caller (best score, global index and R_pred per
pair) as DIR/<name>.npy.  With `--full` the same run also times, as named secondary records: the per-step-collective
cadence (one all-reduce + select per step), weak scaling (50 000 hypotheses PER RANK), BASELINE.json configs[3] (B = 32 x
50 000 split over the ranks), a two-stream variant of the step loop (independent pairs overlap one step's drain with the
next one's ramp) and, at one rank, the shard timings that say what an N-GPU run can reach (`predicted_strong_scaling`).

Launching: `python3 bench.py --gpus N` starts its own N worker processes (one per GPU, RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_* set, rendezvous on 127.0.0.1) BEFORE anything touches a GPU and relays rank 0's JSON
line; under an external launcher (`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`,
which sets RANK / WORLD_SIZE) the process is a worker itself.  `--backend gloo` lets more ranks than GPUs
share the visible device(s): a rehearsal of the multi-rank logic on a 1-GPU box, never a measurement.

Prints ONE JSON line on rank 0 (see the task contract); with `--full` it also carries `roofline` for the fused kernel
(fp32 MFMA bound), the checks of the timed result against the materialised scores, the split-f16 side report and
`cpu_baseline` (the reference's torch-CPU op sequence on the host cores).
"""
import argparse
import importlib
import json
import os
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

N_HYP = 50_000
FLOPS_PER_HYP = 1_839_104      # trilinear 131072 + GEMM1 1572864 + GEMM2 131072 + dot 4096
HBM_BYTES_PER_HYP = 36         # the timed launch keeps only the arg-max (want_scores=False): 36 B of R in
PEAK_F32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: dense fp32 matrix peak (at the 2.4 GHz maximum clock)
MAX_CLOCK_GHZ = 2.4
PEAK_LDS_TBPS = 256 * 256 * 2.4e9 / 1e12   # 157.3: 256 B/clk/CU (ds_read_b128), 256 CUs, 2.4 GHz
SPLIT_LDS_BYTES_PER_HYP = 262144 + 32768 + 98304 + 65536 + 8192   # split-f16 kernel, see its lds_roofline entry
SPLIT_LDS_BYTES_PER_HYP_R3 = 262144 + 32768 + 98304 + 147456 + 8192   # round 3's formulation: every W1 fragment from the LDS
TRAFFIC_JSON = os.path.join("profiles", "traffic.json")


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline: in-kernel clock stamps and event "
                         "brackets in the timed region (roofline), the timed result against the materialised scores, "
                         "the secondary records, the split-f16 side report and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one handed its caller (best_score, best_idx, "
                         "R_pred) as DIR/<name>.npy, float32 / float64")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU baseline")
    ap.add_argument("--split-f16", action="store_true",
                    help="time the opt-in split-f16 kernel (AHV_SCORE_SPLIT_F16) instead of the all-fp32 default; "
                         "by default it is only reported beside the fp32 headline (with --full)")
    ap.add_argument("--prewarm-ms", type=float, default=60.0,
                    help="minimum length of the untimed, time-based pre-warm (the same step, looped until the chip's "
                         "clock has settled: >= this many ms AND three consecutive kernel times within 1 %%; 0 disables)")
    ap.add_argument("--skip-secondary", "--skip-strong-scaling", dest="skip_secondary", action="store_true",
                    help="with --full: leave out the secondary records (profiling runs: they launch the same kernel at "
                         "other shapes, which would mix into rocprofv3's per-kernel averages)")
    ap.add_argument("--backend", default="nccl", help="process-group backend (nccl = RCCL; gloo only to rehearse "
                                                      "the multi-rank logic on a box with fewer GPUs than ranks)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


# ------------------------------------------------------------------------------------------------ parent
def launch_workers(args) -> int:
    """Spawn one fresh worker process per rank (this process has not touched a GPU and never will), relay rank 0's
    stdout (the JSON line), pass stderr through, return the worst exit code."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for rank in range(args.gpus):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), AHV_BENCH_WORKER="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if rank == 0 else subprocess.DEVNULL))
    import threading
    box = {}
    reader = threading.Thread(target=lambda: box.update(out=procs[0].stdout.read().decode()), daemon=True)
    reader.start()
    codes = [None] * len(procs)
    try:
        while any(c is None for c in codes):
            for i, p in enumerate(procs):
                if codes[i] is None:
                    codes[i] = p.poll()
            if any(c not in (None, 0) for c in codes):  # a rank failed: the others would wait in a collective forever
                break
            time.sleep(0.1)
    finally:
        for p in procs:  # exact PIDs we started, only if still alive
            if p.poll() is None:
                p.kill()
        codes = [p.wait() for p in procs]
    reader.join(timeout=10)
    out0 = box.get("out", "")
    sys.stdout.write(out0)
    sys.stdout.flush()
    bad = [c for c in codes if c != 0]
    return bad[0] if bad else 0


# ------------------------------------------------------------------------------------------------ worker
def synth_inputs(ahv, dev, rank):
    """SURVEY.md 8(d) cfg 2: vol ~ N(0, 1.15^2); torch-default conv init for the head; Haar R."""
    import numpy as np
    import torch
    g = torch.Generator().manual_seed(0)
    vol_src = torch.randn(1, 16, 8, 8, 8, generator=g) * 1.15
    vol_tgt = torch.randn(1, 16, 8, 8, 8, generator=g) * 1.15
    W1 = (torch.rand(32, 384, generator=g) * 2 - 1) / np.sqrt(384.0)
    W2 = (torch.rand(32, 32, generator=g) * 2 - 1) / np.sqrt(32.0)
    b2 = (torch.rand(32, generator=g) * 2 - 1) / np.sqrt(32.0)
    R = torch.from_numpy(ahv.rotations.haar_rotations_np(N_HYP, seed=1000))  # ONE set: every rank scores its shard of it
    return [t.to(dev).contiguous() for t in (vol_src, vol_tgt, W1, W2, b2, R)]


def cpu_model_string() -> str:
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or "unknown"


def host_memory_gib() -> float:
    """Memory this process may use: min(MemAvailable, cgroup limit)."""
    avail = float("inf")
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    avail = int(line.split()[1]) / 2 ** 20
    except OSError:
        pass
    for path in ("/sys/fs/cgroup/memory.max", "/sys/fs/cgroup/memory/memory.limit_in_bytes"):
        try:
            v = open(path).read().strip()
            if v != "max":
                avail = min(avail, int(v) / 2 ** 30)
        except (OSError, ValueError):
            pass
    return avail


def host_cpu_share():
    """Threads this process may use: its affinity mask, capped by the cgroup's CPU quota (cpu.max: "<quota> <period>" or
    "max"; v1: cpu.cfs_quota_us / cpu.cfs_period_us).  BASELINE.md section 4 says os.cpu_count(): on a GPU box whose
    container owns a slice of the host that over-subscribes the slice 16-fold, so the share is what is used and all three
    numbers are reported."""
    import math
    affinity = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = int(q) / int(per)
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    threads = affinity if quota is None else max(1, min(affinity, int(math.ceil(quota))))
    return threads, {"os_cpu_count": os.cpu_count(), "sched_affinity": affinity, "cgroup_cpu_quota": quota}


def cpu_baseline(vol_src, vol_tgt, W1, W2, b2, R):
    """the reference's op sequence with stock torch CPU operators (oracle/torch_ref.py) on
    the host cores, same inputs as the GPU run, fp32, no_grad, all host threads of this box's CPU share;
    1 warm-up + best of 3, for BOTH the unchunked call (what the reference does, test_co3d.py:137-140: every
    temporary of all N hypotheses materialised at once, ~130 KB each) and chunks of 1 000 (the fastest variant
    found in the survey).  The unchunked pass needs ~8 GB of host memory at N = 50 000: if the box offers less than
    24 GiB it runs on the first 10 000 hypotheses and says so.  `value` is the faster of the two."""
    import torch
    from oracle import torch_ref
    share, share_info = host_cpu_share()
    cores = int(os.environ.get("AHV_CPU_THREADS", share))
    torch.set_num_threads(cores)
    vs, vt, Rc, w1, w2, bb = [t.cpu() for t in (vol_src, vol_tgt, R, W1, W2, b2)]
    torch_ref.score_hypotheses(vs, vt, Rc[:2000], w1, w2, bb, chunk=1000)  # warm-up (thread pool, oneDNN primitives)

    def best_of(n_hyp, chunk, reps=3, budget_s=25.0):
        times, scores, t_all = [], None, time.perf_counter()
        for _ in range(reps):
            t0 = time.perf_counter()
            scores, _, _ = torch_ref.score_hypotheses(vs, vt, Rc[:n_hyp], w1, w2, bb, chunk=chunk)
            times.append(time.perf_counter() - t0)
            if time.perf_counter() - t_all > budget_s:
                break
        return min(times), len(times), scores

    t_c, reps_c, scores = best_of(N_HYP, 1000)
    n_un = N_HYP if host_memory_gib() >= 24.0 else 10_000
    t_u, reps_u, scores_u = best_of(n_un, None)
    chunked, unchunked = N_HYP / t_c, n_un / t_u
    res = {"value": max(chunked, unchunked), "unit": "hypotheses/s", "cores": torch.get_num_threads(),
           "kind": "port", "cpu_model": cpu_model_string(), "cpu_share": share_info,
           "chunk_1000": {"value": chunked, "seconds": t_c, "n_hyp": N_HYP, "best_of": reps_c},
           "unchunked": {"value": unchunked, "seconds": t_u, "n_hyp": n_un, "best_of": reps_u,
                         "note": "reference-shaped call: all hypotheses materialised at once"},
           "sample": "all %d hypotheses of the same workload (B=1, same tensors as the GPU run), torch %s CPU "
                     "operators, fp32, no_grad, %d threads, 1 warm-up + best of %d: chunks of 1000 %.2f s; "
                     "unchunked (%d hypotheses) %.2f s" % (N_HYP, torch.__version__, torch.get_num_threads(), reps_c,
                                                         t_c, n_un, t_u)}
    assert torch.equal(scores[:, :n_un], scores_u) or (scores[:, :n_un] - scores_u).abs().max().item() < 1e-6
    return res, scores


def kernel_source_sha() -> str:
    """SHA-256 over the sources the fused scorer is compiled from: profiles/traffic.json records the value its PMC passes
    were taken at, and a `traffic` figure from another kernel is not reported."""
    import hashlib
    h = hashlib.sha256()
    for name in ("ahv_score.hip", "ahv_device.h", "ahv_dual.h", "ahv_team.h", "ahv_exact.h", "ahv_split.h"):
        with open(os.path.join(REPO, "3dahv_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def dump_outputs(path, out, dist, use_pg, rank):
    """--dump-outputs: what the last timed step handed its caller, one DIR/<name>.npy per array -- best_score (B,) float32,
    best_idx (B,) float64 (the global index; exact below 2**53), R_pred (B, 3, 3) float32.  Under a process group every rank
    takes part (only the rank whose shard holds the winner has its R_pred row, the others zeros: their sum is that row);
    rank 0 writes."""
    import numpy as np
    R_pred = out["R_pred"].clone()
    if use_pg:
        dist.all_reduce(R_pred, op=dist.ReduceOp.SUM)
    if rank != 0:
        return
    os.makedirs(path, exist_ok=True)
    arrays = {"best_score": out["best"].float(), "best_idx": out["idx"].double(), "R_pred": R_pred.float()}
    for name, t in arrays.items():
        np.save(os.path.join(path, name + ".npy"), t.cpu().numpy())


class VerifyLoop:
    """One rank's verify steps on a fixed workload (the reference's per-pair hot loop, test_co3d.py:137-146):
        step i   = ONE fused launch: forward_3d2d(vol_tgt) + rotate + forward_3d2d + score + running max into its key slot
        finalize = ONE launch per group of `group` steps (8): decode the keys, gather R_pred = proposals[idx], hand the keys
                   back EMPTY
    With a process group the keys of `group` consecutive steps travel in ONE all-reduce(MAX) of group * B int64 words, issued
    in stream order (what a collective costs beside a 0.1 ... 0.7-ms kernel is its fixed part -- the event packets torch
    puts around it, 17 ... 36 us with a one-rank RCCL group, profiles/r04ab_process_group_variants.jsonl -- not its bytes).
    `lanes` > 1: the groups alternate between that many streams, each with its own key buffer and (under a process group)
    its own communicator, so that nothing orders one lane behind the other: independent pairs then overlap one step's
    drain -- the wait for the slowest workgroup, the launch gap, the next prologue -- with the next step's hypotheses."""

    def __init__(self, ops, dist, dev, vol_src, vol_tgt, R_local, head, n_offset, use_pg, group, split, lanes=1):
        import torch
        self.ops, self.dist, self.use_pg = ops, dist, use_pg
        self.group = max(1, group)
        self.vs, self.vt, self.R, self.head, self.n_offset = vol_src, vol_tgt, R_local, head, n_offset
        self.split = split
        self.B = vol_src.shape[0]
        self.lanes = []
        for k in range(max(1, lanes)):
            lane = {"keys": torch.full((self.group, self.B), -(1 << 63), dtype=torch.int64, device=dev),
                    "stream": None, "pg": None, "out": None}
            if lanes > 1:
                lane["stream"] = torch.cuda.Stream(device=dev)
                lane["stream"].wait_stream(torch.cuda.current_stream(dev))  # the inputs above are ready for it
                if use_pg and k > 0:
                    lane["pg"] = dist.new_group(backend=dist.get_backend())  # its own communicator: no order between lanes
            self.lanes.append(lane)
        self.out = {}

    def _finalize(self, lane):
        """In the lane's stream order: (all-reduce of the group's keys,) ONE select for all its steps."""
        keys = lane["keys"]
        if self.use_pg:
            self.dist.all_reduce(keys, op=self.dist.ReduceOp.MAX, group=lane["pg"])
        # with sharding the owner rank holds the winning row, the others get zeros
        best, idx, R_pred = self.ops.select_rotation(keys.view(-1), self.R, n_offset=self.n_offset, reset_key=True)
        B = self.B  # (empty slots of a partial group decode to -inf / -1)
        lane["out"] = (best.view(self.group, B), idx.view(self.group, B), R_pred.view(self.group, B, 3, 3))

    def run(self, steps, brackets=None, stamps=None):
        """`steps` steps, every one finalized on return (the streams are NOT synchronised).  `brackets`: [(first step, last
        step, event, event)] -- HIP events recorded on the launches' own stream in front of launch `first` and behind launch
        `last` (a record idles the queue ~6 us: a bracket spans a whole group of launches and ends before the group's select)."""
        import torch
        before = {b[0]: b[2] for b in (brackets or [])}
        after = {b[1]: b[3] for b in (brackets or [])}
        multi = len(self.lanes) > 1
        main = torch.cuda.current_stream() if multi else None
        lane = self.lanes[0]
        for i in range(steps):
            g, j = divmod(i, self.group)
            if j == 0:
                lane = self.lanes[g % len(self.lanes)]
                if multi:
                    torch.cuda.set_stream(lane["stream"])
            if i in before:
                before[i].record()
            # `stamps` given: the same kernel also writes every workgroup's s_memtime / s_memrealtime pair (shader clock)
            self.ops.verify_pair(self.vs, self.vt, self.R, *self.head, n_offset=self.n_offset, want_scores=False,
                                 best_key=lane["keys"][j], reset_best=False, split_f16=self.split,
                                 clock_stamps=None if stamps is None else stamps[i])
            if i in after:
                after[i].record()
            if j == self.group - 1 or i == steps - 1:  # the group is complete (or the run ends inside it)
                self._finalize(lane)
        if multi:
            torch.cuda.set_stream(main)
            for ln in self.lanes:
                main.wait_stream(ln["stream"])
        j = (steps - 1) % self.group
        best, idx, R_pred = lane["out"]
        self.out = {"best": best[j], "idx": idx[j], "R_pred": R_pred[j]}


def default_lanes(world: int, n_total: int) -> int:
    """Lanes of the step loop a run takes unless AHV_BENCH_LANES says otherwise.  Two lanes pay when a rank's launch is
    SHORT -- the ~18 us of drain, launch gap and prologue that do not shrink with N are then worth overlapping -- and cost
    when it is long: two persistent grids sized for the whole chip then queue for the same CUs.  Measured on one GPU
    (secondary.predicted_strong_scaling): 6 250 hypotheses per rank 0.0988 against 0.1059 ms per step, 12 500: 0.181 / 0.186,
    25 000: 0.404 / 0.352, 50 000: 0.716 / 0.687.  So: two lanes from 4 ranks on (<= AHV_BENCH_TWO_LANES_MAX_N = 16 384
    hypotheses per rank), one lane at 1 and 2 ranks.  The same on every rank (it depends on the world size alone)."""
    if world <= 1:
        return 2 if os.environ.get("AHV_BENCH_TWO_LANES_PG", "0") == "1" else 1
    return 2 if n_total // world <= int(os.environ.get("AHV_BENCH_TWO_LANES_MAX_N", "16384")) else 1


def rank_identity(torch, dev, rank, local_rank, backend):
    """What a reader of a multi-rank line looks for first: which physical GPU each rank drove."""
    p = torch.cuda.get_device_properties(dev)
    bus = None
    if all(hasattr(p, a) for a in ("pci_domain_id", "pci_bus_id", "pci_device_id")):
        bus = "%04x:%02x:%02x.0" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
    else:
        try:  # hipDeviceGetPCIBusId of the runtime torch already loaded
            import ctypes
            buf = ctypes.create_string_buffer(64)
            if ctypes.CDLL("libamdhip64.so").hipDeviceGetPCIBusId(buf, 64, int(dev.index)) == 0:
                bus = buf.value.decode()
        except OSError:
            pass
    coll = None
    if backend == "nccl":
        try:
            coll = "rccl " + ".".join(str(x) for x in torch.cuda.nccl.version())
        except Exception as e:  # noqa: BLE001 -- identity is evidence, never a reason to fail the run
            coll = "rccl (version unavailable: %s)" % type(e).__name__
    else:
        coll = backend
    uuid = getattr(p, "uuid", None)
    return {"rank": rank, "local_rank": local_rank, "device_index": int(dev.index), "device": p.name,
            "gcn_arch": getattr(p, "gcnArchName", None), "pci_bus_id": bus, "uuid": None if uuid is None else str(uuid),
            "host": socket.gethostname(), "pid": os.getpid(), "collectives": coll,
            "visible_devices": os.environ.get("HIP_VISIBLE_DEVICES", os.environ.get("ROCR_VISIBLE_DEVICES"))}


def worker(args):
    import numpy as np
    import torch
    import torch.distributed as dist

    # stdout carries the ONE JSON line and nothing else: libraries that print banners from native code
    # ("[Gloo] Rank 0 is connected ...", RCCL version lines) get stderr for the whole run.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    ndev = torch.cuda.device_count()
    if ndev == 0:
        raise SystemExit("bench.py needs a GPU (no CPU fallback)")
    if args.backend == "nccl" and local_rank >= ndev:
        raise SystemExit("LOCAL_RANK %d but only %d GPU(s) visible (RCCL needs one GPU per rank; --backend gloo "
                         "rehearses more ranks than GPUs)" % (local_rank, ndev))
    dev = torch.device("cuda", local_rank % ndev)  # ranks share a GPU only in a gloo rehearsal
    torch.cuda.set_device(dev)
    # AHV_BENCH_FORCE_PG=1: a single rank still creates the process group and runs every collective of the
    # world > 1 path (key all-reduce ring, barriers, all-gather check) -- the RCCL branch rehearsed on one GPU.
    use_pg = world > 1 or os.environ.get("AHV_BENCH_FORCE_PG", "0") == "1"
    if use_pg:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            sk = socket.socket()
            sk.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
            sk.close()
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)

    ahv = importlib.import_module("3dahv_amd")
    ops, adist = ahv.ops, ahv.dist
    lib = ahv._lib.load()  # fails loudly without the HIP library
    split = bool(args.split_f16)
    # Under a process group the keys of `group` steps share one all-reduce, issued in stream order (DESIGN.md section 6:
    # what a collective costs is the event packets around it, not its bytes; the per-step cadence is timed beside it).
    # The same cadence without a group (one select per 8 steps): pairs are independent, nothing needs a step's winner before
    # the next step starts (the reference appends it to a list, test_co3d.py:152), and N = 1 and N > 1 then time the same loop.
    group = int(os.environ.get("AHV_BENCH_STEPS_PER_COLLECTIVE", "8"))

    vol_src, vol_tgt, W1, W2, b2, R_all = synth_inputs(ahv, dev, rank)
    head = (W1, W2, b2)
    # strong scaling: ONE set of 50 000 hypotheses, this rank's contiguous shard of it
    lo, hi = adist.shard_range(N_HYP, rank, world)
    R, n_offset, n_local = R_all[lo:hi].contiguous(), lo, hi - lo
    # Lanes: where a rank's shard is short (4 ranks and more) the step loop runs on TWO lanes -- groups of steps alternate
    # between two streams, each with its own key buffer and its own communicator, so that one step's drain (the wait for the
    # slowest workgroup, the launch gap, the next prologue: ~18 us that do not shrink with N) overlaps the next step's
    # hypotheses (default_lanes above has the measurements behind the rule).
    # One rank: one lane, one stream -- the N = 1 line is the same measurement as in every earlier round.
    lanes = int(os.environ.get("AHV_BENCH_LANES", str(default_lanes(world, N_HYP))))
    lanes = max(1, min(lanes, 2))
    loop = VerifyLoop(ops, dist, dev, vol_src, vol_tgt, R, head, n_offset, use_pg, group, split, lanes=lanes)
    ncu = lib.ahv_device_cu_count()
    ident = rank_identity(torch, dev, rank, local_rank, args.backend if use_pg else "none")
    ranks_info = [ident]
    if use_pg:
        ranks_info = [None] * world
        dist.all_gather_object(ranks_info, ident)
        if args.backend == "nccl" and world > 1:   # one GPU per rank, every one a different device
            seen = {(r["host"], r["pci_bus_id"] or r["uuid"] or r["device_index"]) for r in ranks_info}
            assert len(seen) == world, "ranks share a GPU: %s" % ranks_info

    def barrier():
        if use_pg:
            dist.barrier()

    def new_events(n):
        return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]

    def group_brackets(steps, grp):
        """HIP-event brackets for the contract's `roofline.kernel_ms`: one bracket per group of `grp` consecutive launches
        of the timed region (first record in front of the group's first launch, second behind its last, BEFORE the group's
        select), every group but the first (step 0 runs behind the barrier's idle gap; a run of one group keeps it).
        A bracket's time / its launches includes the launch gaps between them and amortises the ~6 us a record idles the
        queue over the group, so that kernel_ms <= ms_per_step holds by construction (three single-launch
        brackets at --steps 20 each carried their own record and came out ABOVE ms_per_step)."""
        out = []
        n_groups = (steps + grp - 1) // grp
        for g in range(n_groups):
            first, last = g * grp, min(steps, (g + 1) * grp) - 1
            if g == 0 and n_groups > 1:
                continue
            e0, e1 = new_events(1)[0]
            out.append((first, last, e0, e1))
        return out

    def bracket_ms(brackets):
        """[(ms per launch, launches)] of the brackets (after a synchronize)."""
        return [(b[2].elapsed_time(b[3]) / (b[1] - b[0] + 1), b[1] - b[0] + 1) for b in brackets]

    def prewarm(min_ms, max_ms=1500.0, batch=8):
        """Untimed, TIME-based pre-warm of the same step: the chip needs ~30 ms of this kernel to ramp its clock
        (the first launches after an idle period run ~18 % slower), so a step-count warm-up of a
        0.7-ms kernel sits inside the ramp.  Loops until >= min_ms have elapsed AND the last three kernel times
        agree within 1 % (or max_ms).  Returns what it did, for the JSON line."""
        # every lane runs at least one whole group per batch
        batch = max(batch, loop.group * len(loop.lanes))
        done, last = 0, []
        if use_pg:
            # One batch OUTSIDE the pre-warm's clock: a lane's first collective creates its communicator -- seconds with RCCL
            # across GPUs, during which the chip idles.  Counted against max_ms it ended the pre-warm at once and left the
            # timed region of a short run (20 steps of a 0.1-ms shard) inside the clock ramp.
            loop.run(batch)
            torch.cuda.synchronize()
            dist.barrier()
            torch.cuda.synchronize()
            done += batch
        t0 = time.perf_counter()
        settled = False
        while min_ms > 0:
            evs = new_events(batch)
            loop.run(batch, [(i, i, a, b) for i, (a, b) in enumerate(evs)])
            torch.cuda.synchronize()
            done += batch
            last = (last + [a.elapsed_time(b) for a, b in evs])[-3:]
            elapsed = (time.perf_counter() - t0) * 1e3
            settled = len(last) == 3 and (max(last) - min(last)) <= 0.01 * min(last)
            stop = (elapsed >= min_ms and settled) or elapsed >= max_ms or min_ms <= 0
            if use_pg:  # every rank must run the same number of steps (each carries a collective): stop together
                flag = torch.tensor([1 if stop else 0], dtype=torch.int32, device=dev)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                stop = bool(flag.item())
            if stop:
                break
        return {"prewarm_ms": (time.perf_counter() - t0) * 1e3, "prewarm_steps": done, "prewarm_settled": settled,
                "prewarm_last_kernel_ms": [round(x, 4) for x in last]}

    def timed(lp, steps, warmup, brackets=None, stamps=None):
        """W untimed steps, then exactly `steps` steps between barrier + synchronize on both sides; MAX over ranks."""
        if warmup:
            lp.run(warmup)
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lp.run(steps, brackets, stamps)
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        if use_pg:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def global_best(scores, offset):
        """torch.max over the materialised scores of ALL ranks: (value, global index) per sample."""
        lv, li = torch.max(scores, dim=1)
        cand = torch.stack([lv.double(), (li + offset).double()], dim=1)  # (B, 2)
        if use_pg:
            allc = [torch.zeros_like(cand) for _ in range(world)]
            dist.all_gather(allc, cand)
            cand = torch.stack(allc)  # (world, B, 2)
            # largest value, lowest index among equals
            order = torch.argsort(cand[:, :, 1], dim=0)
            cand = torch.gather(cand, 0, order[:, :, None].expand_as(cand))
            pick = torch.argmax(cand[:, :, 0], dim=0)
            cand = cand[pick, torch.arange(cand.shape[1], device=cand.device)]
        return cand

    def headline(dt, pre, out):
        """The fields of every result line: what a plain run prints; --full adds its records to them."""
        return {
            "metric": "rotation hypotheses scored/sec (B=1)", "value": N_HYP * args.steps / dt, "unit": "hypotheses/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f16 hi/lo split products, f32 accumulate" if split else "f32",
            "data": "synthetic",
            **pre,
            "config": {"workload": "CO3D pair (BASELINE.json configs[1]): B=1, ONE set of N_hyp=50000 Haar rotations split "
                                   "over the GPUs (contiguous shards, n_offset), source volume 16x8x8x8 (P=512 voxel sites x "
                                   "16 ch), head 384->32->32, 64 positions",
                       "n_hyp_per_gpu": n_local, "n_hyp_total": N_HYP,
                       "parallelism": "hypothesis axis sharded x%d, 8-byte key all-reduce(max)" % world,
                       "backend": "single process" if not use_pg else ("rccl" if args.backend == "nccl" else args.backend),
                       "step": "ONE fused launch (forward_3d2d(tgt) + rotate + forward_3d2d + score + arg-max: "
                               "ahv_verify_pair_f32)%s + ONE select launch per %d step(s) (decode + gather R_pred + key reset)" % (
                                   " + ONE all-reduce(MAX) of the int64 keys of %d steps, in stream order" % loop.group
                                   if use_pg else "", loop.group),
                       "steps_per_collective": loop.group if use_pg else None, "steps_per_select": loop.group,
                       "lanes": lanes,
                       "lanes_note": None if lanes == 1 else "groups of %d steps alternate between %d streams, each with its own "
                                     "key buffer and its own communicator: independent pairs overlap one step's drain with the "
                                     "next step's hypotheses (AHV_BENCH_LANES=1 for the one-stream loop; with --full, secondary."
                                     "n50k_b1_one_stream times it in this run)" % (loop.group, lanes),
                       "ranks": ranks_info},
            # what the timed region computed (with --full asserted against torch.max over the materialised scores of
            # all ranks): lets a forced-process-group run be compared with a single-process run
            "result": {"best_idx": int(out["idx"].item()), "best_score": float(out["best"].item())},
        }

    # The cyclic garbage collector stays off from here to the end of the measurements: a generation-2 collection inside an
    # issue loop is a multi-millisecond host stall (the queue runs dry), and one BETWEEN the pre-warm and the timed steps
    # idles the GPU long enough to drop its clock (seen: the first 16 timed launches at 0.82 ... 0.70 ms).
    import gc
    gc.collect()
    gc.disable()
    with torch.no_grad():
        pre = prewarm(args.prewarm_ms)
        if not args.full:
            # a plain run: the step loop alone between the barriers -- no event brackets, no in-kernel clock stamps, nothing
            # measured or checked after it
            dt = timed(loop, args.steps, args.warmup)
            gc.enable()
            out = dict(loop.out)
            if args.dump_outputs:
                dump_outputs(args.dump_outputs, out, dist, use_pg, rank)
            if rank == 0:
                os.write(json_fd, (json.dumps(headline(dt, pre, out)) + "\n").encode())
            if use_pg:
                dist.destroy_process_group()
            return
        stamps = torch.zeros(args.steps, 4 * ncu, dtype=torch.int64, device=dev)
        if lanes == 1:
            # fused kernel, HIP events on its stream, inside the timed region
            brackets = group_brackets(args.steps, loop.group)
            dt = timed(loop, args.steps, args.warmup, brackets, stamps)
            kern_src = "HIP events on the kernel's stream INSIDE the timed region: one bracket per group of %d launches " \
                       "(first group left out), time / launches" % loop.group
        else:
            # Two lanes: consecutive launches overlap, so an event pair around a launch would time the overlap, not the
            # kernel.  The timed region carries no events; `roofline.achieved` is priced from the WALL time (flops x steps /
            # timed seconds) and kernel_ms comes from a ONE-LANE calibration leg of the same step in front of it.
            cal = VerifyLoop(ops, dist, dev, vol_src, vol_tgt, R, head, n_offset, use_pg, group, split, lanes=1)
            cal_steps = max(2 * cal.group, min(args.steps, 48))
            brackets = group_brackets(cal_steps, cal.group)
            cal_dt = timed(cal, cal_steps, 0, brackets)
            dt = timed(loop, args.steps, args.warmup, None, stamps)
            kern_src = "one-lane calibration leg (%d steps, same shard, same collectives, %.4f ms per step) in front of the " \
                       "two-lane timed region: HIP events per group of %d launches" % (cal_steps, cal_dt / cal_steps * 1e3, cal.group)
        out = dict(loop.out)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, out, dist, use_pg, rank)
        kern_pairs = bracket_ms(brackets)
        kern_list = [ms for ms, _ in kern_pairs]
        kern_ms = float(sum(ms * n for ms, n in kern_pairs) / sum(n for _, n in kern_pairs))
        # shader clock held DURING the timed launches: per workgroup (s_memtime delta) / (s_memrealtime delta at
        # 100 MHz); median over workgroups and launches (MI355X_MICROARCH.md "DVFS give-back" item 6)
        st_all = stamps.cpu().numpy().reshape(args.steps, -1, 4)
        st = st_all.reshape(-1, 4)
        st = st[st[:, 3] > st[:, 1]]
        clock_ghz = float(np.median((st[:, 2] - st[:, 0]) / (st[:, 3] - st[:, 1]))) * 0.1 if len(st) else None
        # every timed launch from its own workgroups' 100-MHz real-time stamps: first hypothesis-loop entry -> last exit
        # (the ~5 us of per-workgroup prologue and the launch itself are outside these stamps)
        loop_ms = []
        for row in st_all:
            row = row[row[:, 3] > row[:, 1]]
            if len(row):
                loop_ms.append(float(row[:, 3].max() - row[:, 1].min()) * 1e-5)

        # correctness of what was timed: the merged key equals torch.max over the materialised scores of ALL ranks, and
        # (sharded runs) the winner of the UNSHARDED set scored on this rank alone -- exactly: a score does not depend on
        # how the set is cut (a team's score is a lone wave's bit for bit, csrc/ahv_team.h)
        scores, key = ops.verify_pair(vol_src, vol_tgt, R, *head, n_offset=n_offset, split_f16=split)
        gbest = global_best(scores, n_offset)[0]
        assert int(out["idx"].item()) == int(gbest[1].item()), (out["idx"], gbest)
        assert float(out["best"].item()) == float(gbest[0].item())
        if world > 1:
            s_all, k_all = ops.verify_pair(vol_src, vol_tgt, R_all, *head, split_f16=split)
            assert torch.equal(s_all[:, lo:hi], scores)
            v_all, i_all = torch.max(s_all, dim=1)
            assert int(out["idx"].item()) == int(i_all.item()) and float(out["best"].item()) == float(v_all.item())

        # ---- secondary records, same run, same timing (barriers, max over ranks)
        def leg(vs, vt, R_set, steps, warmup, grp=None, lanes=1, shard=True, offset=None):
            """`steps` verify steps of (vs, vt) against R_set -- sharded over the ranks (shard=True: a FIXED total) or whole
            on every rank -- timed like the headline."""
            n_total = R_set.shape[0]
            a, b = adist.shard_range(n_total, rank, world) if shard else (0, n_total)
            off = a if offset is None else offset
            lp = VerifyLoop(ops, dist, dev, vs, vt, R_set[a:b].contiguous(), head, off, use_pg, group if grp is None else grp,
                            split, lanes=lanes)
            t = timed(lp, steps, warmup)
            B = vs.shape[0]
            total = n_total if shard else n_total * world
            return lp, {"n_hyp_total": total, "B": B, "n_hyp_per_rank": b - a, "steps": steps, "warmup": warmup,
                        "steps_per_collective": lp.group if use_pg else None, "steps_per_select": lp.group, "lanes": lanes,
                        "ms_per_step": t / steps * 1e3, "hypotheses_per_s": B * total * steps / t, "pairs_per_s": B * steps / t}

        sec_steps = max(24, min(args.steps, 96))
        g = torch.Generator().manual_seed(5)
        vs32 = (torch.randn(32, 16, 8, 8, 8, generator=g) * 1.15).to(dev)
        vt32 = (torch.randn(32, 16, 8, 8, 8, generator=g) * 1.15).to(dev)
        secondary = None
        if not args.skip_secondary:
            secondary = {"note": "same step, same collectives, timed between barriers, max over ranks; 48 untimed steps in "
                                 "front of each leg (the checks before it let the clock sag)"}
            # the per-step cadence: ONE all-reduce + ONE select per verify step (test_co3d.py:145-146 as written)
            lp1, secondary["n50k_b1_collective_per_step"] = leg(vol_src, vol_tgt, R_all, sec_steps, 48, grp=1)
            assert int(lp1.out["idx"].item()) == int(out["idx"].item())
            # weak scaling: 50 000 hypotheses PER RANK (rounds 1-4's headline), each rank its own set
            R_own = torch.from_numpy(ahv.rotations.haar_rotations_np(N_HYP, seed=1000 + rank)).to(dev)
            _, secondary["weak_n50k_per_rank_b1"] = leg(vol_src, vol_tgt, R_own, sec_steps, 48, shard=False, offset=rank * N_HYP)
            # BASELINE.json configs[3]: B = 32 pairs x 50 000 shared hypotheses split over the ranks
            lp3, secondary["configs3_b32_n50k"] = leg(vs32, vt32, R_all, 5, 2)
            s32, _ = ops.verify_pair(vs32, vt32, R_all, *head, split_f16=split)
            assert torch.equal(lp3.out["idx"], torch.max(s32, dim=1)[1])
            del s32
            # the other lane count: a run on one lane times two lanes beside its headline; a run on two lanes (4 ranks and more by
            # default, each lane its own communicator) times the one-stream loop beside it
            if lanes == 1:
                lp2, secondary["n50k_b1_two_lanes"] = leg(vol_src, vol_tgt, R_all, 2 * sec_steps, 48, grp=max(group, 4), lanes=2)
            else:
                lp2, secondary["n50k_b1_one_stream"] = leg(vol_src, vol_tgt, R_all, sec_steps, 48, lanes=1)
            assert int(lp2.out["idx"].item()) == int(out["idx"].item())
            if world == 1:
                # what a strong-scaling run can reach, from this GPU alone: the shard a rank of an n-GPU run scores per
                # step (contiguous 1/n of the same set, n_offset, the multi-rank cadence of 8 steps per select, no
                # collective), one lane and two
                pred = {"note": "t(50 000) / (n * t(50 000 / n)) on ONE GPU, 8 steps per select, no collective: the efficiency an "
                                "n-GPU strong-scaling run can reach before link latency"}
                t_ref = {}
                pred_steps = 96   # independent of --steps: at the driver's 20 steps these legs scattered by +-5 %
                pred_lanes = (1, 2, 3) if os.environ.get("AHV_BENCH_PRED_THREE_LANES", "0") == "1" else (1, 2)
                suffix = {1: "", 2: "_two_lanes", 3: "_three_lanes"}
                for nl in pred_lanes:
                    _, r = leg(vol_src, vol_tgt, R_all, pred_steps if nl == 1 else 2 * pred_steps, 48, grp=8, lanes=nl)
                    t_ref[nl] = r["ms_per_step"]
                for n in (2, 4, 8):
                    a, b = adist.shard_range(N_HYP, n - 1, n)   # the last rank's shard (offsets included)
                    row = {"n_hyp_per_rank": b - a}
                    for nl in pred_lanes:
                        _, r = leg(vol_src, vol_tgt, R_all[a:b], 2 * pred_steps, 48, grp=8, lanes=nl, offset=a)
                        row["ms_per_step" + suffix[nl]] = r["ms_per_step"]
                        row["efficiency" + suffix[nl]] = t_ref[nl] / (n * r["ms_per_step"])
                        # what the driver computes: the N-rank value over N times the ONE-rank, one-lane value
                        row["efficiency_vs_one_lane_n1" + suffix[nl]] = t_ref[1] / (n * r["ms_per_step"])
                    # ... for the lane count a --gpus n run takes by default (default_lanes)
                    row["default_lanes"] = default_lanes(n, N_HYP)
                    row["efficiency_default"] = row["efficiency_vs_one_lane_n1" + suffix[row["default_lanes"]]]
                    pred["n_gpus_%d" % n] = row
                pred["ms_per_step_n50k"] = t_ref[1]
                pred["ms_per_step_n50k_two_lanes"] = t_ref[2]
                secondary["predicted_strong_scaling"] = pred
        feat_tgt = ops.forward_3d2d(vol_tgt, W1, W2, b2)  # for the split-f16 side report below
    gc.enable()

    if rank == 0:
        value = N_HYP * args.steps / dt                      # the whole job: ONE set of 50 000 hypotheses per step
        if lanes == 1:
            achieved = FLOPS_PER_HYP * n_local / (kern_ms * 1e-3) / 1e12   # the timed kernel scores this rank's shard
        else:   # overlapping launches: this rank's algorithmic flops of the timed region / its wall time
            achieved = FLOPS_PER_HYP * n_local * args.steps / dt / 1e12
        per_step = None if secondary is None else secondary["n50k_b1_collective_per_step"]
        # HBM bytes per launch: NOT measured in this run (PMC passes need rocprofv3) -- the committed figure of
        # tools/profile_bench.sh on the same command, reported only while it describes THIS kernel and THIS launch shape:
        # the hash of the scorer's sources must equal the one recorded with the counters (else null + the reason), the
        # launch must be the 50 000-hypothesis one the counters were taken on, and the figure must cover at least what
        # the launch has to read (a WRITE_SIZE / FETCH_SIZE mix-up or a unit slip would fall below it).
        traffic, traffic_src = None, None
        tpath = os.path.join(REPO, TRAFFIC_JSON)
        if os.path.exists(tpath):
            with open(tpath) as f:
                tj = json.load(f)
            sha = kernel_source_sha()
            if tj.get("kernel_src_sha") != sha:
                traffic_src = {"stale": "the scorer's sources changed since the PMC passes of %s (sha %s..., now %s...): "
                                        "re-run tools/profile_bench.sh" % (tj.get("source"), str(tj.get("kernel_src_sha"))[:12], sha[:12])}
            elif n_local != N_HYP:
                traffic_src = {"not_applicable": "counters were taken on the 50 000-hypothesis launch; this rank scores %d" % n_local}
            else:
                traffic = tj.get("fused_hbm_bytes_per_launch")
                assert traffic >= HBM_BYTES_PER_HYP * N_HYP, "traffic.json below the algorithmic bytes: wrong counter or unit"
                traffic_src = {"bytes": traffic, "source": tj.get("source"), "source_commit": tj.get("source_commit"),
                               "kernel_src_sha": sha, "formula": tj.get("formula"),
                               "note": "rocprofv3 --pmc passes of the same command; not measured in this run"}
        kname = "score_hypotheses_dual_kernel<false, true>"
        res = headline(dt, pre, out)
        res.update({
            # the reference's literal cadence (test_co3d.py:145-146: torch.max + proposals[idx] after EVERY pair; with ranks,
            # one all-reduce per step too), timed in the same run on one stream; `value` amortises the select (and the
            # collective) over `steps_per_select` independent pairs -- the same cadence at every N
            "ms_per_step_select_every_step": None if per_step is None else per_step["ms_per_step"],
            "value_select_every_step": None if per_step is None else per_step["hypotheses_per_s"],
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / PEAK_F32_MFMA_TFLOPS, "traffic": traffic, "traffic_source": traffic_src,
                         "kernel": kname, "kernel_ms": kern_ms,
                         "kernel_ms_min": float(np.min(kern_list)), "kernel_ms_median": float(np.median(kern_list)),
                         "kernel_ms_mean": kern_ms, "kernel_ms_per_bracket": [round(x, 4) for x in kern_list],
                         "kernel_ms_is": kern_src + " (%d brackets, %d launches)" % (len(kern_pairs), sum(n for _, n in kern_pairs)),
                         "achieved_is": "algorithmic flops per launch / kernel_ms" if lanes == 1 else
                                        "this rank's algorithmic flops of the timed region / its wall time (launches overlap)",
                         "hypothesis_loop_ms_all_launches_median": float(np.median(loop_ms)) if loop_ms else None,
                         "hypothesis_loop_ms_is": "in-kernel s_memrealtime stamps of ALL %d timed launches: first workgroup "
                                                  "entering its hypothesis loop -> last leaving it" % args.steps,
                         "frac_at_median": FLOPS_PER_HYP * n_local / (float(np.median(kern_list)) * 1e-3) / 1e12
                                           / PEAK_F32_MFMA_TFLOPS,
                         "algorithmic_flops_per_launch": FLOPS_PER_HYP * n_local,
                         "algorithmic_flops_note": "%d hypotheses (this rank's shard) x 1 839 104; the in-launch target "
                                                   "features (one more forward_3d2d per workgroup) are NOT counted" % n_local,
                         "algorithmic_hbm_bytes_per_launch": HBM_BYTES_PER_HYP * n_local,
                         "shader_clock_ghz": clock_ghz,
                         "shader_clock_source": "s_memtime / s_memrealtime stamps of the TIMED launches (all %d, all "
                                                "workgroups, median)" % args.steps,
                         "frac_at_delivered_clock": (achieved / (PEAK_F32_MFMA_TFLOPS * clock_ghz / MAX_CLOCK_GHZ)
                                                     if clock_ghz else None)},
            "secondary": secondary,
        })
        if split:  # opt-in kernel: priced against the f16 matrix peak (16 x the fp32 one)
            res["roofline"].update(kernel="forward_3d2d_small_kernel + score_hypotheses_dual_kernel<true, false>",
                                   peak=16 * PEAK_F32_MFMA_TFLOPS,
                                   frac=achieved / (16 * PEAK_F32_MFMA_TFLOPS), frac_at_delivered_clock=None,
                                   traffic=None, traffic_source=None,
                                   note="GEMM1 runs 3 f16 MFMA products per algorithmic MAC; the kernel is bound by "
                                        "LDS bandwidth (trilinear gather), not by the matrix pipe")
        if world == 1 and not split:
            # The opt-in split-f16 kernel on the same inputs, reported beside the fp32 headline (never as `value`).
            with torch.no_grad():
                s4, k4 = ops.score_hypotheses(vol_src, feat_tgt, R, W1, W2, b2, split_f16=True)

                k0 = loop.lanes[0]["keys"][0]

                def split_launch(ev=None):
                    if ev is not None:
                        ev[0].record()
                    ops.score_hypotheses(vol_src, feat_tgt, R, W1, W2, b2, want_scores=False, best_key=k0,
                                         reset_best=False, split_f16=True)
                    if ev is not None:
                        ev[1].record()
                t_pre = time.perf_counter()  # the same time-based pre-warm as the headline kernel (clock ramp)
                while (time.perf_counter() - t_pre) * 1e3 < max(args.prewarm_ms, 1.0):
                    for _ in range(16):
                        split_launch()
                    torch.cuda.synchronize()
                ev = new_events(50)
                for e in ev:
                    split_launch(e)
                torch.cuda.synchronize()
            ms4 = float(np.median([a.elapsed_time(b) for a, b in ev]))
            res["split_f16_kernel"] = {
                "note": "AHV_SCORE_SPLIT_F16 (opt-in, per-call flag): GEMM1 as 3 f16 MFMA products of hi/lo split "
                        "operands, f32 accumulate",
                "kernel_ms": ms4, "kernel_ms_is": "median of 50 launches after the time-based pre-warm",
                "hypotheses_per_s_kernel_only": N_HYP / (ms4 * 1e-3),
                "max_abs_score_diff_vs_f32_kernel": float((s4 - scores).abs().max().item()),
                "same_argmax": bool(torch.equal(ops.unpack_best(k4)[1], ops.unpack_best(key)[1])),
                # its real roof is the LDS, not the f16 matrix pipe (288 f16 MFMAs per hypothesis ~ 15 % of the time):
                # bytes one hypothesis moves through the LDS in this formulation / the guide's LDS rate
                "lds_roofline": {"bound": "lds", "bytes_per_hypothesis": SPLIT_LDS_BYTES_PER_HYP,
                                 "bytes_breakdown": "gather 8 voxels x 8 corners x 4 ds_read_b128 per lane 262144 + image "
                                                    "stores 32768 + B fragments 98304 + W1 fragments 65536 (64 of the 144 "
                                                    "fragment reads; the other 80 are served from registers) + target 8192",
                                 "achieved": SPLIT_LDS_BYTES_PER_HYP * N_HYP / (ms4 * 1e-3) / 1e12,
                                 "peak": PEAK_LDS_TBPS, "unit": "TB/s",
                                 "frac": SPLIT_LDS_BYTES_PER_HYP * N_HYP / (ms4 * 1e-3) / 1e12 / PEAK_LDS_TBPS,
                                 # the same time priced with the bytes of round 3's formulation (what the 0.47 of
                                 # rounds 3 was quoted on): comparable across rounds, not a statement about LDS traffic
                                 "frac_at_round3_bytes": SPLIT_LDS_BYTES_PER_HYP_R3 * N_HYP / (ms4 * 1e-3) / 1e12 / PEAK_LDS_TBPS,
                                 "note": "peak = 256 B/clk/CU x 256 CUs x 2.4 GHz (MI355X_MICROARCH.md, LDS); bank "
                                         "conflicts of the rotated gather (1.64 LDS cycles per conflict-free cycle, "
                                         "simulated and measured) are inside the achieved figure"}}
        if world == 1 and not args.no_cpu_baseline:
            cb, cpu_scores = cpu_baseline(vol_src, vol_tgt, W1, W2, b2, R)
            res["cpu_baseline"] = cb
            # same inputs, same answers: scores <= 1e-4 relative, arg-max exact
            gpu_scores = scores.cpu()
            rel = ((gpu_scores - cpu_scores).abs() / cpu_scores.abs().clamp_min(1e-2)).max().item()
            assert rel < 1e-4, rel
            assert int(torch.argmax(cpu_scores, dim=1).item()) == int(torch.argmax(gpu_scores, dim=1).item())
            res["cpu_baseline"]["gpu_vs_cpu_max_rel_err"] = rel
            res["cpu_baseline"]["gpu_speedup_over_chunk_1000"] = value / cb["chunk_1000"]["value"]
            res["cpu_baseline"]["gpu_speedup_over_unchunked"] = value / cb["unchunked"]["value"]
        os.write(json_fd, (json.dumps(res) + "\n").encode())
    if use_pg:
        dist.destroy_process_group()


def main():
    args = parse_args()
    external = "RANK" in os.environ and "WORLD_SIZE" in os.environ  # torch.distributed.run or our own parent
    if args.gpus > 1 and not external:
        sys.exit(launch_workers(args))
    worker(args)


if __name__ == "__main__":
    main()
