#!/usr/bin/env python3
"""bench.py - headline benchmark of the se2lam hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W          (N>1: launched by torch.distributed.run, or - when no
                                                            WORLD_SIZE is set - bench.py starts the N ranks itself)
    python bench.py ... --dump-outputs DIR                 (also writes the last timed step's results as DIR/*.npy)
    python bench.py ... --full                             (also every other leg: see below)

Metric (BASELINE.json): BA Gauss-Newton/LM iterations per second on the 200-keyframe /
20k-landmark synthetic SE(2) graph (config 4 formulation = Map::loadLocalGraph applied to a
whole-map window), timed over exactly K steps after W warm-up steps.  A plain run
does only that.  With --full the same JSON line also carries a sustained sample of the headline
graph (at least SE2_BENCH_MIN_TIMED_S seconds), the per-kernel pass and roofline, the batched
local windows, ORB extract+match frames/s at 640x480 (the `orb` object) and the CPU baselines.

A "step" is ONE LM outer iteration (linearise -> Schur reduction -> dense pose solve ->
back-substitution/update -> chi^2, incl. any retry trials) of the reference's protocol
optimize(10) (Config::LOCAL_ITER, LocalMapper.cpp:260): K steps = ceil(K/10) optimize() calls on
the graph resident in HBM, estimates reset (device-to-device) before each call.
N>1: landmarks are sharded over the ranks (poses replicated), the fused buffer [S | b | scalars]
is summed with one RCCL all-reduce per LM trial (+ one 4-double all-reduce for the trial cost);
total work is fixed -> "scaling": "strong".
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (MI355X_MICROARCH.md: 8.0 TB/s spec, ~6.3 TB/s achievable)
ITERS_PER_CALL = 10    # Config::LOCAL_ITER of the synthetic setup
MIN_TIMED_S = float(os.environ.get("SE2_BENCH_MIN_TIMED_S", "2.0"))   # (the profiling captures of tools/capture.sh shorten it) floor of the --full sustained sample of the headline graph (long enough for a 5 s SMI sampler to see the device busy)
DUMP_MAX_BYTES = 64 << 20  # --dump-outputs: larger landmark arrays are written as a fixed, seeded sample of rows
MIN_WINDOWS_S = min(0.4, MIN_TIMED_S)    # ... of every row of the window sweep (its best row is then timed again for MIN_TIMED_S)
FP64_PEAK_TFLOPS = 78.6   # MI355X FP64 vector = matrix peak (MI355X_MICROARCH.md)


_T0 = time.time()


def log(msg):
    """progress on stderr (stdout carries only the JSON line): a hang is then attributable to a section"""
    print(f"[bench {time.time() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


def cgroup_cpu_quota():
    """CPUs the cgroup grants (cpu.max of cgroup v2 / cfs quota of v1), None when unlimited or unknown"""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
        if q != "max":
            return max(1, int(int(q) / int(per) + 0.5))
    except (OSError, ValueError):
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            q = int(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            per = int(f.read())
        if q > 0:
            return max(1, int(q / per + 0.5))
    except (OSError, ValueError):
        pass
    return None


def host_cores():
    """cores this process can really use: the affinity mask, capped by the cgroup's CPU quota (the GPU boxes show 256
    hardware threads and grant 16 CPUs - 256 runnable threads are then throttled to a fraction of one thread each)"""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    q = cgroup_cpu_quota()
    return min(n, q) if q else n


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kf", type=int, default=200)
    ap.add_argument("--landmarks", type=int, default=20000)
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: sustained sample, per-kernel pass and roofline, BA windows, ORB and CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the poses, landmarks and chi2 history of the last timed step as DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-orb", action="store_true")
    ap.add_argument("--orb-batch", type=int, default=256)
    ap.add_argument("--orb-steps", type=int, default=10)
    ap.add_argument("--orb-inflight", type=int, default=3,
                    help="ORB batches in flight on the resident leg (extractor handles on their own streams, taking turns); 1 = one "
                         "handle.  Three since round 5: 201-203 k frames/s against 193-194 k with two (the third batch fills what the "
                         "latency-bound tail of a batch leaves idle); the PCIe-inclusive leg keeps two (its copies need the other queues)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--ba-mixed", type=int, default=1, help="0: skip the batch of distinct windows of the window leg")
    ap.add_argument("--ba-windows", type=int, default=-1,
                    help="independent 50-KF local windows optimised concurrently per GPU (se2gpu_ba_optimize_batch); "
                         "-1 = sweep 1, 8, 32, 64; 0 = skip")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def _free_port():
    import socket
    for _ in range(64):
        with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        try:   # the rendezvous listens on MASTER_PORT + 1 (torchrun's own store owns MASTER_PORT): that one must be free too
            with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s2:
                s2.bind(("127.0.0.1", port + 1))
            return port
        except OSError:
            continue
    return 29500


def spawn_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves, one process per GPU, with the environment
    torch.distributed.run would give them (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT).  Rank 0's stdout is
    ours (the JSON line); the other ranks' stdout goes to stderr.  Returns the worst exit code."""
    import subprocess
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), SE2_BENCH_SPAWNED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: what RCCL needs across processes on this driver
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=None if r == 0 else sys.stderr))
    rc = 0
    try:
        for p in procs:
            rc = max(rc, abs(p.wait()))
    except BaseException:
        for p in procs:   # exactly the processes started here
            if p.poll() is None:
                p.kill()
        raise
    return rc


def _dry_run(rank, world):
    """SE2_BENCH_DRY_RUN=1: the launch + rendezvous skeleton of an N-rank run without touching a GPU (the CPU test of the
    self-spawn path): every rank joins the TCP rendezvous, rank 0's 128-byte token reaches all of them, timings are maxed."""
    from se2lam_amd.rendezvous import Rendezvous
    dist = Rendezvous(rank, world)
    token = bytes((7 * i + 3) % 251 for i in range(128))
    got = dist.broadcast(token if rank == 0 else None, 128)
    ok = 1.0 if got == token else 0.0
    worst = dist.allreduce_max(1.0 - ok)               # 0.0 iff every rank received the token
    top = dist.allreduce_max(float(rank))
    dist.barrier()
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "token_ok": worst == 0.0, "max_rank": int(top),
                          "spawned": os.environ.get("SE2_BENCH_SPAWNED") == "1"}), flush=True)
    dist.close()


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no launcher around us: become one (VERDICT r02 missing #3)
        if os.environ.get("SE2_BENCH_DRY_RUN") != "1":
            from se2lam_amd import capi
            have = capi.device_count()
            if have < args.gpus:
                raise SystemExit(f"bench.py --gpus {args.gpus}: only {have} device(s) visible (one rank per GPU)")
        raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        log(f"--gpus {args.gpus} but WORLD_SIZE={world}: the launcher's world size wins")
        args.gpus = world
    if os.environ.get("SE2_BENCH_DRY_RUN") == "1":
        return _dry_run(rank, world)

    from se2lam_amd import capi, synth
    from se2lam_amd.optimizer import SlamOptimizer

    if capi.device_count() == 0:
        raise SystemExit("bench.py needs a GPU: libse2gpu has no CPU fallback")
    if world > 1 and capi.device_count() <= local_rank:
        raise SystemExit(f"rank {rank}: LOCAL_RANK {local_rank} but only {capi.device_count()} device(s) visible "
                         f"(one rank per GPU)")

    dist = None      # se2lam_amd.rendezvous.Rendezvous when N > 1
    torch = None     # never imported: see se2lam_amd/rendezvous.py (two HSA runtimes cannot share a process)
    comm = None
    # N>1: the data-path collective is RCCL, called by libse2gpu itself on its own HIP stream (se2gpu_comm_*).  The only
    # things exchanged outside it are the 128-byte ncclUniqueId, barriers and the max of the timings (TCP, stdlib).
    # SE2_BENCH_FORCE_DIST=1 runs that code path with a single rank (the only way to exercise it on a 1-GPU box).
    use_dist = world > 1 or os.environ.get("SE2_BENCH_FORCE_DIST") == "1"
    capi.check(capi.lib().se2gpu_set_device(local_rank if use_dist else 0))
    if use_dist:
        import ctypes as C
        from se2lam_amd.rendezvous import Rendezvous
        dist = Rendezvous(rank, world)
        uid = np.zeros(128, np.uint8)
        with _stdout_to_stderr():   # RCCL prints a "Librccl path" banner on stdout; stdout carries only the JSON line
            if rank == 0:
                capi.check(capi.lib().se2gpu_comm_unique_id(uid.ctypes.data))
            uid = np.frombuffer(dist.broadcast(uid.tobytes(), 128), np.uint8).copy()
            comm = C.c_void_p()
            capi.check(capi.lib().se2gpu_comm_create(uid.ctypes.data, rank, world, C.byref(comm)))
            nranks = C.c_int(-1)
            capi.check(capi.lib().se2gpu_comm_count(comm, C.byref(nranks)))
        if nranks.value != world:   # ncclCommCount: what RCCL itself says the communicator spans
            raise SystemExit(f"rank {rank}: the RCCL communicator spans {nranks.value} ranks, expected {world}")

    def sync_all():
        capi.check(capi.lib().se2gpu_device_synchronize())   # hipDeviceSynchronize (= torch.cuda.synchronize())
        if dist is not None:
            dist.barrier()
            capi.check(capi.lib().se2gpu_device_synchronize())

    log(f"rank {rank}/{world}: building the BA graph")
    # ---------------- workload: BA graph resident in HBM ----------------
    g_full = synth.ba_graph(args.kf, args.landmarks)
    g = g_full.shard(rank, world)
    opt = SlamOptimizer()
    if use_dist:
        opt.set_comm(comm)          # landmark shard rank/world + native RCCL all-reduce of [S | b | scalars]
    opt.load(g)
    opt.initializeOptimization(0)

    def run_steps(k):
        done = 0
        trials = 0
        while done < k:
            it = min(ITERS_PER_CALL, k - done)
            opt.reset_estimates()
            got = opt.optimize(it)
            if got != it:
                raise SystemExit(f"LM stopped after {got}/{it} iterations: {opt.stats}")
            trials += opt.stats["trials"]
            done += it
        return trials

    log("BA: warm-up")
    run_steps(args.warmup)
    # Warm-up continues, untimed, until nothing one-off is left for the timed region: optimize(n) is captured into a
    # hipGraph the SECOND time a shape n is asked of a handle and replayed from the third (12 ms of capture would otherwise
    # land inside a 40 ms sample - VERDICT r02 weak #6).  The shapes the timed loop uses: ITERS_PER_CALL and the remainder.
    for shape in {min(ITERS_PER_CALL, args.steps), args.steps % ITERS_PER_CALL}:
        for _ in range(3 if shape else 0):
            opt.reset_estimates()
            opt.optimize(shape)
    # The timed region is exactly K steps: `steps` in the JSON is what ran and what was asked.
    sync_all()
    t0 = time.perf_counter()
    trials = run_steps(args.steps)
    sync_all()
    dt = time.perf_counter() - t0
    if dist is not None:
        dt = dist.allreduce_max(dt)
    steps = args.steps
    iters_per_s = steps / dt
    chi2_final = opt.stats["chi2_final"]
    if args.dump_outputs:
        _dump_outputs(args.dump_outputs, opt, "" if world == 1 else f".rank{rank}")
    log(f"BA: {iters_per_s:.1f} it/s over {steps} steps")

    sustained = roofline = exchange = windows_obj = orb_obj = cpu = None
    if args.full:
        # The same graph over whole blocks of K steps, never shorter than MIN_TIMED_S of device work (20 steps of this graph
        # are 4 ms).  The number of blocks comes from the headline sample (every rank computes the same count from the
        # all-reduced time); should the sample still come out short, it is taken again with more blocks - the floor is
        # enforced, not estimated.
        blocks = max(1, int(np.ceil(1.25 * MIN_TIMED_S / max(dt, 1e-6))))
        while True:
            s_steps = args.steps * blocks
            sync_all()
            t0 = time.perf_counter()
            for _ in range(blocks):
                run_steps(args.steps)
            sync_all()
            s_dt = time.perf_counter() - t0
            if dist is not None:
                s_dt = dist.allreduce_max(s_dt)
            if s_dt >= MIN_TIMED_S:
                break
            blocks *= 2
        sustained = {"iters_per_s": s_steps / s_dt, "steps": s_steps, "timed_s": s_dt, "ms_per_step": 1e3 * s_dt / s_steps}
        log(f"BA: {s_steps / s_dt:.1f} it/s over {s_steps} steps (sustained); per-kernel pass")
        # ---------------- per-kernel durations with HIP events on the kernels' stream ----------------
        # Same K steps again with an event pair around every launch (serialises the stream, so it is a
        # separate pass and not the timed region above).
        opt.profile(True)
        run_steps(min(s_steps, 50))
        sync_all()
        prof = opt.profile_report()
        opt.profile(False)
        kern = {k: {"avg_us": 1e3 * ms / max(n, 1), "launches": n, "total_ms": ms} for k, (ms, n) in prof.items()}
        # the dominant KERNEL: the exchange of the sharded run ("allreduce_*", timed like a launch) is reported beside it
        only_k = {k: v for k, v in kern.items() if not k.startswith("allreduce")}
        dom = max(only_k, key=lambda k: only_k[k]["total_ms"]) if only_k else None
        if use_dist:
            per_iter = lambda name: (kern[name]["total_ms"] * 1e3 / max(kern["k_chol_tiles"]["launches"], 1)
                                     if name in kern and "k_chol_tiles" in kern else None)   # noqa: E731
            exchange = {"what": "RCCL all-reduce (sum, f64) of the packed lower-triangular tiles of [S | b] + scalars, once per "
                                "LM trial, on the handle's stream; per-kernel pass (event pair around every call)",
                        "doubles_per_trial": opt.exchange_doubles(),   # of the (possibly re-ordered, padded) system this handle factorises
                        "comm_ranks": int(nranks.value),
                        "allreduce_system_us": kern.get("allreduce_system", {}).get("avg_us"),
                        "allreduce_small_us": kern.get("allreduce_small", {}).get("avg_us"),
                        "pack_unpack_us": kern.get("k_tri_pack", {}).get("avg_us"),
                        "allreduce_us_per_iteration": (per_iter("allreduce_system") or 0.0) + (per_iter("allreduce_small") or 0.0)
                        if "k_chol_tiles" in kern else None}
        B_ba = g_full.algorithmic_bytes_per_iter()
        B_ba_rank = g.algorithmic_bytes_per_iter()

        def kernel_bytes(name):
            """Algorithmic bytes ONE launch of `name` has to move; whole-iteration figure otherwise."""
            n3 = 3 * g.P
            if name.startswith("k_chol"):       # dense pose solve: lower triangle of S + rhs in, x out
                return 8 * (n3 * (n3 + 1) // 2 + n3) + 8 * n3
            if name == "k_reduce2":             # 152 B per contributor pair + the reduced system written once
                k = np.bincount(np.asarray(g.e_lm), minlength=g.L).astype(np.int64)
                return int(152 * (k * (k - 1) // 2).sum() + 8 * n3 * n3)
            if name == "k_linearize":
                return 44 * g.E + 24 * g.L + 24 * g.P + 216 * g.E + 144 * g.L
            if name in ("k_update", "k_finalize"):
                return 44 * g.E + 72 * g.E + 48 * g.L + 24 * g.L
            return B_ba_rank
        traffic = _pmc_traffic()
        if dom is not None:
            avg_s = kern[dom]["avg_us"] * 1e-6
            B_dom = kernel_bytes(dom)
            achieved = B_dom / avg_s / 1e9
            roofline = {
                "bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS,
                # HBM bytes per launch of that kernel from rocprofv3 PMC passes (profiles/pmc_traffic.json, collected with
                # tools/pmc_summarize.py on this workload; FETCH_SIZE x2 correction) - null when the file has no entry
                "traffic": (_traffic_of(traffic, dom)[0] if world == 1 else None),
                "traffic_commit": traffic.get("_meta", {}).get("commit"),
                "traffic_code_sha": traffic.get(dom, {}).get("code_sha"),
                "traffic_stale": _traffic_of(traffic, dom)[1],
                "algorithmic_bytes_per_launch": B_dom, "avg_launch_us": kern[dom]["avg_us"],
                "note": ("the dominant kernel is the dense pose solve: a 600-column dependency chain, bound by FP64 / LDS "
                         "latency and inter-workgroup hand-offs, not by bandwidth (DESIGN.md 4.1, 7)"
                         if dom.startswith("k_chol") else None),
                "whole_step_achieved": B_ba * iters_per_s / 1e9,
                "whole_step_frac": B_ba * iters_per_s / 1e9 / HBM_PEAK_GBS,
                "kernels_us": {k: round(v["avg_us"], 3) for k, v in kern.items()},
            }
            if dom.startswith("k_chol"):
                # what the solve IS bound by, in numbers: its FP64 work against the part's FP64 rate, and the length of
                # the dependency chain against the launch time - neither bytes nor flops limit it, the chain of pivots does
                n3 = 3 * g.P
                flops = n3 ** 3 / 3.0 + 4.0 * n3 * n3          # LDL^T of the augmented system + the two triangular solves
                roofline["fp64"] = {"flops_per_launch": flops, "achieved_tflops": flops / avg_s / 1e12, "peak_tflops": FP64_PEAK_TFLOPS,
                                    "frac": flops / avg_s / 1e12 / FP64_PEAK_TFLOPS}
                roofline["bound_by"] = {"what": "latency: a chain of dependent pivots", "pivots": n3,
                                        "ns_per_pivot": 1e9 * avg_s / n3}

    # ---------------- batched local windows: the machine filled (SURVEY.md section 7 hard part 6) ----------------
    if args.full and args.ba_windows != 0:
        log("BA windows leg")
        try:
            windows_obj = _ba_windows(args, rank, world, sync_all, dist)
        except Exception as exc:   # never takes the headline down
            windows_obj = {"error": repr(exc)}

    # ---------------- ORB leg (frames/s) ----------------
    if args.full and not args.no_orb:
        log("ORB leg")
        try:
            from se2lam_amd import orb_bench
            own_process = world == 1 and args.orb_inflight > 2    # the PCIe-inclusive leg with the two handles of a streaming caller
            orb_obj = orb_bench.run(rank, world, args.orb_batch, args.orb_steps, sync_all, dist, torch,
                                    traffic=traffic if args.orb_batch == 256 else {}, inflight=args.orb_inflight,
                                    streaming_leg=not own_process)
            if own_process and orb_obj is not None:
                log("ORB streaming leg (own process)")
                orb_obj["streaming"] = _in_subprocess("orb_streaming", {"batch": args.orb_batch, "steps": 40},
                                                      timeout=180.0)
        except ImportError:
            orb_obj = None
        log("ORB leg done; CPU baselines")
        if orb_obj is not None and rank == 0 and world == 1 and not args.no_cpu_baseline:
            orb_obj["cpu_baseline"] = _orb_cpu_baseline(synth, args.orb_batch)

    # ---------------- CPU baseline (rank 0, N=1 only): the oracle on the host cores ----------------
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        log("BA CPU baseline")
        cpu = _ba_cpu_baseline(g_full, args.cpu_seconds)
        log("pipeline (configs[0]) CPU baseline")
        cpu["pipeline"] = _pipeline_baseline()
        log("done")

    if rank == 0:
        out = {
            "metric": "BA GN-iters/s (200 KF, 20k pts)", "value": iters_per_s, "unit": "iters/s",
            "n_gpus": world, "steps": steps, "steps_requested": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / steps, "timed_s": dt, "sustained": sustained,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic",
            # the figure that CAN scale with N: every rank optimises its own independent windows, no collective (north_star:
            # "independent keyframe windows shard across the GPUs"); `value` above is the strong-scaling form of ONE window,
            # whose replicated dense solve caps it
            "value_weak": (windows_obj or {}).get("value"), "scaling_weak": "weak",
            "metric_weak": (windows_obj or {}).get("metric"),
            "config": {"workload": f"globalBA-window {g_full.P} KF / {g_full.L} landmarks / {g_full.E} EdgeSE2XYZ "
                                   f"+ {g_full.O} PreEdgeSE2, LM optimize(10) (config 4 formulation, SURVEY D3)",
                       "parallelism": f"landmark-sharded x{world}, RCCL all-reduce of [S|b]" if world > 1 else "single GPU",
                       "lm_trials_per_step": trials / steps, "chi2_final": chi2_final,
                       # the other two legs' headline figures, where a reader of `parsed` finds them (their full objects follow below)
                       "orb_frames_per_s": (orb_obj or {}).get("value"),
                       "orb_roofline_frac": ((orb_obj or {}).get("roofline") or {}).get("frac"),
                       "orb_valu_issue_frac": (((orb_obj or {}).get("roofline") or {}).get("valu") or {}).get("frac"),
                       "orb_whole_step_frac": ((orb_obj or {}).get("roofline") or {}).get("whole_step_frac"),
                       "ba_windows_iters_per_s": (windows_obj or {}).get("value"),
                       "ba_windows_in_flight": ((windows_obj or {}).get("best") or {}).get("windows_per_gpu"),
                       "ba_windows_path": ((windows_obj or {}).get("best") or {}).get("path")},
            "roofline": roofline,
            "exchange": exchange,
            "cpu_baseline": cpu,
            "ba_windows": windows_obj,
            "orb": orb_obj,
        }
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        del opt
        with _stdout_to_stderr():
            capi.lib().se2gpu_comm_destroy(comm)
        dist.close()


def _dump_outputs(out_dir, opt, suffix=""):
    """--dump-outputs: what a caller of the timed path receives from its last optimize() - the pose and landmark estimates
    (this rank's shard when N > 1) and the chi2 after every iteration - as float64 DIR/<name><suffix>.npy.  Landmarks that
    would take the files past DUMP_MAX_BYTES are written as a fixed, seeded sample of rows, `landmarks_rows` their indices."""
    os.makedirs(out_dir, exist_ok=True)
    poses, lms = opt.estimates()
    out = {"poses": poses, "chi2_hist": np.asarray(opt.stats["chi2_hist"], np.float64)}
    room = DUMP_MAX_BYTES - sum(a.nbytes + 4096 for a in out.values()) - 2 * 4096     # (4096: an .npy header, generously)
    if lms.nbytes > room:
        k = room // (lms.itemsize * lms.shape[1] + 8)
        rows = np.sort(np.random.default_rng(0).choice(len(lms), size=k, replace=False))
        out["landmarks"], out["landmarks_rows"] = lms[rows], rows.astype(np.float64)
    else:
        out["landmarks"] = lms
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + suffix + ".npy"), np.ascontiguousarray(a, np.float64))


def _ba_windows(args, rank, world, sync_all, dist, P=50, L=5000, calls=6):
    """N independent local-BA windows (BASELINE config 3: 50 KF / 5k landmarks / ~30k edges, optimize(10)) in flight at once
    on every GPU: one handle + stream per window, all LM controllers on the device (se2gpu_ba_optimize_batch).  A single
    window leaves > 95 % of the chip idle; this is the throughput form north_star's "independent keyframe windows shard
    across the GPUs" describes - no collective, weak scaling over ranks.  Reports aggregate LM iterations/s and the
    whole-step HBM fraction per window count."""
    from se2lam_amd import synth
    from se2lam_amd.optimizer import SlamOptimizer, optimize_batch, reset_estimates_batch
    g = synth.ba_graph(P, L)
    B = g.algorithmic_bytes_per_iter()
    counts = [args.ba_windows] if args.ba_windows > 0 else [1, 8, 32, 64, 128, 256]
    opts = []
    rows = []
    for n in counts:
        while len(opts) < n:
            o = SlamOptimizer()
            o.load(g)
            o.initializeOptimization(0)
            opts.append(o)
        cur = opts[:n]

        def run():
            reset_estimates_batch(cur)      # one launch (128 one-by-one copies cost the host more than the batch costs the device)
            its = optimize_batch(cur, ITERS_PER_CALL)
            return sum(its)

        def timed(floor_s):
            run()
            sync_all()
            t0 = time.perf_counter()
            done = 0
            reps = 0
            while reps < calls or time.perf_counter() - t0 < floor_s:
                done += run()
                reps += 1
            sync_all()
            dt = time.perf_counter() - t0
            if dist is not None:   # weak form: every rank ran its own windows, no collective; the job's rate = all ranks' iterations / slowest rank's time
                dt = dist.allreduce_max(dt)
                done = int(dist.allreduce_sum(float(done)))
                rate = done / dt
            else:
                rate = done / dt
            return {"windows_per_gpu": n, "iters_per_s": rate, "ms_per_optimize10": 1e3 * dt / reps, "timed_s": dt,
                    "path": _batch_path_name(),
                    "whole_step_achieved_gbs": B * rate / world / 1e9,
                    "whole_step_frac": B * rate / world / 1e9 / HBM_PEAK_GBS}

        rows.append(timed(MIN_WINDOWS_S))
        log(f"BA windows x{n}: {rows[-1]['iters_per_s']:.0f} it/s aggregate ({rows[-1]['path']})")
        if n == counts[-1] or len(counts) == 1:
            # the sweep's best count again, for the full floor (the rows above are 0.4 s samples)
            nb = max(rows, key=lambda r: r["iters_per_s"])["windows_per_gpu"]
            cur = opts[:nb]
            n = nb
            best = timed(MIN_TIMED_S)
            log(f"BA windows x{nb}, {best['timed_s']:.1f} s: {best['iters_per_s']:.0f} it/s aggregate ({best['path']})")
    mixed = None
    if args.ba_mixed and (args.ba_windows <= 0 or args.ba_windows >= 16):
        # the same batch size with DISTINCT windows (30-60 key frames, 3-6 k landmarks, different seeds, a few starts that
        # reject trials): sizes, solve plans and accept / reject patterns differ per window - the honest form of the number above
        nmix = args.ba_windows if args.ba_windows > 0 else int(best["windows_per_gpu"])   # (the sweep's best count)
        gs = synth.mixed_windows(nmix)
        mopts = []
        for gm in gs:
            o = SlamOptimizer()
            o.load(gm)
            o.initializeOptimization(0)
            mopts.append(o)

        def run_mixed():
            reset_estimates_batch(mopts)
            its = optimize_batch(mopts, ITERS_PER_CALL)
            return sum(its), sum(i * gm.algorithmic_bytes_per_iter() for i, gm in zip(its, gs)), sum(o.stat("trials") for o in mopts)

        run_mixed()
        sync_all()
        t0 = time.perf_counter()
        done = byts = trials = reps = 0
        while reps < calls or time.perf_counter() - t0 < 2 * MIN_WINDOWS_S:
            a, b, c = run_mixed()
            done += a; byts += b; trials += c; reps += 1
        sync_all()
        dt = time.perf_counter() - t0
        if dist is not None:
            dt = dist.allreduce_max(dt)
            done = int(dist.allreduce_sum(float(done)))
            byts = dist.allreduce_sum(float(byts)) / world
        mixed = {"windows_per_gpu": nmix, "iters_per_s": (done if dist is not None else world * done) / dt, "lm_trials_per_iter": trials / max(done, 1),
                 "ms_per_optimize10": 1e3 * dt / reps, "whole_step_achieved_gbs": byts / dt / 1e9,
                 "whole_step_frac": byts / dt / 1e9 / HBM_PEAK_GBS, "path": _batch_path_name(),
                 "key_frames": [min(gm.P for gm in gs), max(gm.P for gm in gs)], "landmarks": [min(gm.L for gm in gs), max(gm.L for gm in gs)],
                 "edges_total": int(sum(gm.E for gm in gs)), "windows_with_rejected_trials": int(sum(1 for o in mopts if max(o.stats["trials_hist"]) > 1))}
        log(f"BA windows x{nmix} (distinct windows): {mixed['iters_per_s']:.0f} it/s aggregate, {mixed['lm_trials_per_iter']:.2f} trials per iteration")
        del mopts
    traffic = _pmc_traffic()
    tw = traffic.get("k_window_lm")
    if tw and tw.get("windows_per_launch"):
        # HBM bytes of ONE LM iteration of one window on the resident path, from the PMC capture of tools/capture.sh (its launches hold
        # `windows_per_launch` uniform windows, ITERS_PER_CALL iterations each, plus the two opening passes of an optimize())
        per_it = tw["traffic_bytes"] / (tw["windows_per_launch"] * ITERS_PER_CALL)
        best["resident_traffic"] = {"bytes_per_window_iteration": per_it, "algorithmic_bytes_per_iter": B, "ratio": per_it / B,
                                    "code_sha": tw.get("code_sha")}
    return {"metric": "BA LM-iters/s, independent 50-KF windows in flight", "value": best["iters_per_s"],
            "unit": "iters/s", "n_gpus": world, "scaling": "weak",
            "config": {"workload": f"localBA window {g.P} KF / {g.L} landmarks / {g.E} EdgeSE2XYZ + {g.O} PreEdgeSE2, "
                                   f"LM optimize(10), N windows concurrently per GPU (no collective)",
                       "algorithmic_bytes_per_iter": B},
            "best": best, "sweep": rows, "mixed": mixed}


def _batch_path_name():
    """which path the last se2gpu_ba_optimize_batch of this thread took"""
    try:
        from se2lam_amd import capi
        return {0: "one stream per window", 1: "lock step (one launch per stage for all windows)",
                2: "resident (one workgroup per window, csrc/ba_window.hip)"}.get(int(capi.lib().se2gpu_ba_last_batch_path()), "?")
    except Exception:   # noqa: BLE001
        return "?"


def _ba_cpu_baseline(g, seconds):
    """The CPU path timed on this box's host cores: (i) the 1-thread port (the reference's LocalMapper is
    one thread, g2o is built without OpenMP) and (ii) the all-core variant oracle/ba_ref_mt.cpp (OpenMP over landmarks /
    pose rows, LAPACK dpotrf for the pose solve when scipy's is reachable) in the best of a few thread counts.  The
    headline `value` is the faster of the two; both are reported."""
    from oracle import oracle
    oracle.lib()
    what = f"{g.P} KF / {g.L} landmark / {g.E} edge graph"

    def timed(fn, budget):
        t1 = time.perf_counter()
        n_it = 0
        while True:
            _, _, st = fn()
            n_it += st["iterations"]
            if time.perf_counter() - t1 >= budget:
                break
        return n_it / (time.perf_counter() - t1), n_it

    v1, n1 = timed(lambda: oracle.ba_optimize(g, ITERS_PER_CALL, 0), 0.4 * seconds)
    single = {"value": v1, "unit": "iters/s", "cores": 1, "kind": "port",
              "sample": f"{n1} LM iterations ({n1 // ITERS_PER_CALL} x optimize(10)) of the same {what}, "
                        f"oracle/ba_ref.cpp, 1 thread"}
    out = dict(single)
    multi = _in_subprocess("ba", {"P": g.P, "L": g.L, "seconds": 0.5 * seconds}, timeout=max(60.0, 6 * seconds))
    if "value" in multi:
        multi["sample"] = multi["sample"].replace("GRAPH", what)
        if multi["value"] > v1:
            out = dict(multi)
    out["all_cores"] = multi
    out["single_thread"] = single
    out["host"] = _host_desc()
    return out


def _orb_cpu_baseline(synth, nframes, seconds=10.0):
    """oracle extract + MatchByWindow on a bounded sample of the same synthetic sequence: 1 thread (the reference's Track
    thread; cv::FAST is serial) and frame-parallel over all host cores (ctypes releases the GIL)."""
    from oracle import oracle
    imgs = synth.frames(min(nframes, 256))   # bounded by `seconds`, not by the number of frames
    t1 = time.perf_counter()
    nfr = 0
    prev = oracle.orb_extract(imgs[0])
    while time.perf_counter() - t1 < 0.5 * seconds and nfr < len(imgs) - 1:
        cur = oracle.orb_extract(imgs[nfr + 1])
        oracle.match_window(prev[0], prev[1], cur[0], cur[1])
        prev = cur
        nfr += 1
    cdt = time.perf_counter() - t1
    single = {"value": nfr / cdt, "unit": "frames/s", "cores": 1, "kind": "port",
              "sample": f"{nfr} frames of the same synthetic sequence: oracle/orb_ref.cpp extract + "
                        f"oracle/match_ref.cpp MatchByWindow, 1 thread"}
    out = dict(single)
    reference = _orb_reference_baseline(imgs, 0.3 * seconds)
    multi = _in_subprocess("orb", {"nframes": len(imgs), "seconds": 0.4 * seconds}, timeout=max(60.0, 6 * seconds))
    if "value" in multi and multi["value"] > single["value"]:
        out = dict(multi)
    out["all_cores"] = multi
    out["single_thread"] = single
    out["reference"] = reference
    out["host"] = _host_desc()
    return out


def _orb_reference_baseline(imgs, seconds):
    """The reference ITSELF where it compiles: oracle/_ref = /root/reference/src/ORBextractor.cpp +
    ORBmatcher.cpp + Frame.cpp, unmodified (ORBextractor::operator() :727-788, MatchByWindow :278-381), one thread, the same
    frames.  The OpenCV calls underneath (FAST, resize, GaussianBlur, retainBest) are the stand-in's scalar code, not OpenCV's
    SIMD builds - hence the kind."""
    try:
        from oracle import ref
        if not ref.available():
            return {"error": "oracle/_ref is not built here"}
        ref.lib()
        t1 = time.perf_counter()
        nfr = 0
        prev = ref.orb_extract(imgs[0])
        while time.perf_counter() - t1 < seconds and nfr < len(imgs) - 1:
            cur = ref.orb_extract(imgs[nfr + 1])
            ref.match_window(prev[0], prev[1], cur[0], cur[1])
            prev = cur
            nfr += 1
        cdt = time.perf_counter() - t1
        return {"value": nfr / cdt, "unit": "frames/s", "cores": 1, "kind": "reference sources, 3P = stand-in",
                "sample": f"{nfr} frames: the reference's own ORBextractor::operator() + ORBmatcher::MatchByWindow (oracle/_ref, "
                          f"compiled from /root/reference unmodified, OpenCV stand-in underneath), 1 thread"}
    except Exception as exc:   # test infrastructure: never take the bench line down
        return {"error": repr(exc)}


def _in_subprocess(which, cfg, timeout):
    """The all-core CPU legs run in a child process with a hard timeout: hundreds of OpenMP / OpenBLAS threads on a
    box whose cgroup grants fewer cores can take minutes, and a C call cannot be interrupted from Python."""
    import subprocess
    env = dict(os.environ, OMP_WAIT_POLICY="passive", OMP_PROC_BIND="false")
    if which == "orb_streaming":
        # a streaming process gives every stream a hardware queue of its own (the default of four is dealt in creation order and
        # puts the upload stream behind an extractor's: 100 k frames/s in a fresh process, 155 k with 32 queues); the resident
        # leg is the other way round (202 k with four queues, 185 k with eight or more) and keeps the default in this process
        env.setdefault("GPU_MAX_HW_QUEUES", "32")
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-child", which, json.dumps(cfg)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
        lines = [l for l in r.stdout.decode(errors="replace").splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:
            return {"error": f"child rc {r.returncode}: {r.stderr.decode(errors='replace')[-300:]}"}
        return json.loads(lines[-1])
    except subprocess.TimeoutExpired:
        return {"error": f"all-core leg did not finish within {timeout:.0f} s (killed)"}


def _cpu_child(which, cfg):
    if which == "orb_streaming":   # (a GPU leg: the ORB pipeline with the transfers in the loop, in a process of its own)
        from se2lam_amd import orb_bench
        with _stdout_to_stderr():
            out = orb_bench.streaming_child(int(cfg["batch"]), int(cfg["steps"]))
        print(json.dumps(out), flush=True)
        return
    if which == "pipeline":
        with _stdout_to_stderr():
            out = _pipeline_child(cfg["kind"], int(cfg["frames"]), int(cfg["fps"]))
        print(json.dumps(out), flush=True)
        return
    from oracle import oracle
    from se2lam_amd import synth
    oracle.lib()
    ncore = host_cores()
    if which == "ba":
        g = synth.ba_graph(cfg["P"], cfg["L"])
        seconds = cfg["seconds"]

        def timed(fn, budget):
            t1 = time.perf_counter()
            n_it = 0
            while True:
                _, _, st = fn()
                n_it += st["iterations"]
                if time.perf_counter() - t1 >= budget:
                    break
            return n_it / (time.perf_counter() - t1), n_it

        best = None
        for thr in sorted({ncore, max(1, ncore // 2), min(ncore, 64), min(ncore, 16)}, reverse=True):
            for lap in (True, False):
                oracle.ba_optimize_mt(g, 2, thr, lap)                       # warm the thread pools
                v, _ = timed(lambda: oracle.ba_optimize_mt(g, ITERS_PER_CALL, thr, lap), 0.05 * seconds)
                if best is None or v > best[0]:
                    best = (v, thr, lap)
        v, thr, lap = best
        vm, nm = timed(lambda: oracle.ba_optimize_mt(g, ITERS_PER_CALL, thr, lap), 0.6 * seconds)
        print(json.dumps({"value": vm, "unit": "iters/s", "cores": thr, "kind": "port",
                          "sample": f"{nm} LM iterations of the same GRAPH, oracle/ba_ref_mt.cpp: OpenMP x{thr} over "
                                    f"landmarks / pose rows, pose solve by "
                                    f"{'LAPACK dpotrf (scipy OpenBLAS)' if lap else 'scalar LL^T'}; best of thread counts "
                                    f"up to {ncore} usable cores"}), flush=True)
    else:
        from concurrent.futures import ThreadPoolExecutor
        imgs = synth.frames(cfg["nframes"])
        thr = min(ncore, len(imgs))

        def extract(t):
            return oracle.orb_extract(imgs[t])

        with ThreadPoolExecutor(thr) as ex:
            list(ex.map(extract, range(min(thr, 8))))          # warm-up
            t1 = time.perf_counter()
            done = 0
            while time.perf_counter() - t1 < cfg["seconds"]:
                # the GPU pipeline's shape: every frame extracted once (frame-parallel), then frame t matched with t + 1
                ft = list(ex.map(extract, range(len(imgs))))
                list(ex.map(lambda t: oracle.match_window(ft[t][0], ft[t][1], ft[t + 1][0], ft[t + 1][1]), range(len(imgs) - 1)))
                done += len(imgs)
            cdt = time.perf_counter() - t1
        print(json.dumps({"value": done / cdt, "unit": "frames/s", "cores": thr, "kind": "port",
                          "sample": f"{done} frames: oracle extract of every frame, then MatchByWindow t -> t+1, both "
                                    f"frame-parallel over {thr} threads (= usable cores)"}), flush=True)


def _pipeline_child(kind, nframes, fps):
    """BASELINE.json configs[0], timed: the reference's own Track -> LocalMapper -> optimizer (compiled from /root/reference where the
    sources lie, oracle/_ref; fed frame by frame by oracle/ref_pipeline_driver.cpp) over `nframes` synthetic frames + odometry.
    kind "cpu": every source the reference's, one thread (its Track and LocalMapper are one thread each); kind "dropin": the same
    sources with ORBextractor.cpp / ORBmatcher.cpp replaced by the bindings over libse2gpu and optimize() forwarded to it."""
    from oracle import pipeline
    from se2lam_amd import synth
    if not pipeline.available(kind):
        return {"error": "oracle/_ref/libse2lam_pipeline_%s.so is not built here" % kind}
    frames, odo = synth.frames(nframes), pipeline.odometry(nframes)
    cfg = pipeline.default_config()
    cfg.fps = fps
    if kind == "dropin":    # first-use costs (code objects, arenas) stay out of the sample, as they do for every other GPU leg
        pipeline.run(kind, frames[:12], odo[:12], cfg, raw_matches=False)
    res = pipeline.run(kind, frames, odo, cfg, raw_matches=False)
    ms = res["ms_track"] + res["ms_mapper"]
    bas = [r for r in res["frames"] if r["local_ba"]]
    return {"value": 1e3 * nframes / ms, "unit": "frames/s", "cores": 1,
            "kind": "reference sources, 3P = stand-in" if kind == "cpu" else "reference sources over libse2gpu",
            "ms_per_frame_track": res["ms_track"] / nframes,
            "ms_per_local_ba": (sum(r["ms_mapper"] for r in bas) / len(bas)) if bas else None,
            "key_frames_inserted": int(sum(r["new_kf"] for r in res["frames"])), "local_bas": len(bas),
            "map_points": int(res["frames"][-1]["n_mps"]),
            "sample": f"{nframes} synthetic 640x480 frames + SE(2) odometry through the reference's Track::mTrack -> LocalMapper::addNewKF / "
                      f"localBA -> optimizer (key frame at most every {fps + 1} frames), one thread; "
                      + ("ORBextractor / ORBmatcher / g2o optimize() / findFundamentalMat = the reference's sources and the OpenCV / g2o stand-ins"
                         if kind == "cpu" else
                         "ORBextractor / ORBmatcher = tests/dropin bindings over libse2gpu, optimize() and findFundamentalMat forwarded to it; "
                         "host buffers in and out every call (PCIe-inclusive)")}


def _pipeline_baseline(nframes=60, fps=10):
    """cpu_baseline.pipeline: configs[0]'s CPU run timed beside the same run over libse2gpu (both in child processes)"""
    cpu = _in_subprocess("pipeline", {"kind": "cpu", "frames": nframes, "fps": fps}, timeout=240.0)
    gpu = _in_subprocess("pipeline", {"kind": "dropin", "frames": nframes, "fps": fps}, timeout=240.0)
    out = dict(cpu)
    out["over_libse2gpu"] = gpu
    if "value" in cpu and "value" in gpu:
        out["speedup_end_to_end"] = gpu["value"] / cpu["value"]
    return out


class _stdout_to_stderr:
    """temporarily route file descriptor 1 to stderr (C libraries that print banners on stdout)"""

    def __enter__(self):
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        import ctypes
        ctypes.CDLL(None).fflush(None)   # C stdio buffers of the library (the banner) go to stderr as well
        os.dup2(self._saved, 1)
        os.close(self._saved)


def source_sha():
    """sha256 over the kernel sources (csrc/*.hip, *.h, *.inc): what a PMC capture is valid for.  The GPU box has no
    .git, so the capture is stamped with this instead of (and next to) the commit hash."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "se2lam_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h", ".inc")):
            h.update(f.encode())
            with open(os.path.join(d, f), "rb") as fh:
                h.update(fh.read())
    return h.hexdigest()[:16]


def _pmc_traffic():
    """profiles/pmc_traffic.json (tools/pmc_summarize.py), kernel by kernel: an entry counts only if the DEVICE CODE it was
    measured on is the device code this library carries - every entry is stamped with the hash of its kernel's gfx950 code
    object (se2lam_amd/devcode.py), read back from libse2gpu.so here.  A host-only edit of a source file, or a change in
    another translation unit, leaves a kernel's entry valid; a change of its own code object drops it (roofline.traffic =
    null, traffic_stale = true for that kernel).  (Rounds 2-4 stamped the whole csrc/ directory: any edit staled everything.)"""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            t = json.load(f)
    except (OSError, ValueError):
        return {}
    meta = dict(t.get("_meta", {}))
    try:
        from se2lam_amd import devcode
        now = devcode.kernel_code_hashes()
    except Exception as exc:   # unreadable library: nothing can be vouched for
        return {"_meta": dict(meta, stale=True, stale_reason=repr(exc))}
    out, stale = {}, []
    for k, v in t.items():
        if k == "_meta":
            continue
        ours = not k.startswith("__amd_")   # a runtime kernel such as __amd_rocclr_copyBuffer is not ours to hash
        if isinstance(v, dict) and v.get("code_sha") and ((not ours and k not in now) or (k in now and v["code_sha"] == now[k])):
            out[k] = v
        else:
            stale.append(k)     # (also: a kernel of ours that is no longer in the library, and every entry when the library's code
                                #  objects could not be read at all - an empty hash map vouches for nothing)
    out["_meta"] = dict(meta, stale_kernels=stale, stale=bool(not now))
    return out


def _traffic_of(traffic, kernel):
    """(bytes per launch or None, is the capture stale for this kernel?)"""
    e = traffic.get(kernel)
    meta = traffic.get("_meta", {})
    if e:
        return e.get("traffic_bytes"), False
    return None, bool(meta.get("stale")) or kernel in meta.get("stale_kernels", [])


def _host_desc():
    model = "?"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"nproc": os.cpu_count(), "cgroup_cpu_quota": cgroup_cpu_quota(), "usable_cores": host_cores(), "cpu": model}


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--cpu-child":
        _cpu_child(sys.argv[2], json.loads(sys.argv[3]))
    else:
        main()
