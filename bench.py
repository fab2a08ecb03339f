#!/usr/bin/env python3
"""bench.py -- straggler-detection scoring throughput on MI355X.

Metric (BASELINE.json): duration samples/s reduced to perf scores; report latency at
4096 ranks.  One "step" = one full report over synthetic integer-ns durations already
resident in HBM: per-kernel stats (HIP) -> per-kernel best-rank reference -> per-rank
relative + individual weighted scores -> straggler sets, landed on the host.

Workload (value): BASELINE configs[1] per GPU -- 64 simulated ranks x 2048 kernels x
10,000 pushed samples, the last 8192 retained (the reference ring cap).  With N GPUs the
kernel columns are sharded by hash(kernel name) % N with 2048*N kernels in total (weak
scaling); the only exchange is one RCCL all_gather of [64][6] f64 score partials.
Secondary: report latency at 4096 ranks (configs[2]: 4096 x 2048 x 1024 samples, the
same 2048 kernels split over the N GPUs), and configs[3]: Zipf record streams at 16,384
simulated ranks (47,482 {slot, ns} records per rank, kernel k pushed floor(8192/k^1.1)
times, 1.3x stragglers) -> bucket by slot -> length-classed stats -> scores.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
A plain run sets up, warms up, times the K steps of the value workload and prints the line with
the headline figure (value, ms_per_step).  --full adds everything else to the line: the same loop
with the default host wait, the statistics kernel's roofline, the one-report-at-a-time launch
mode, the secondary legs, the CPU baselines and the drop-in API (--no-* switches apply there).
--dump-outputs DIR writes the results of the last timed step (scores, straggler masks, error
word) as DIR/<name>.npy; the inputs are seeded, so two builds can be compared output for output.
N > 1: one process per GPU over RCCL.  Under torchrun (WORLD_SIZE set) every process is one
rank; run directly with --gpus N > 1, this script starts `torch.distributed.run
--nproc-per-node N` on itself as a CHILD process (before anything touches the GPU) and exits
with its status.  NVRX_BENCH_BACKEND=gloo: rehearsal of the multi-rank path with every rank on
GPU 0 and the partials exchanged over gloo (never a reported number); --dry-run: the launcher
and rendezvous only (no GPU work; CPU test of the launcher).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "nvidia-resiliency-ext-x_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nvidia_resiliency_ext.straggler import batch, ops, synth  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, MI355X_MICROARCH.md chip table (spec)
THR = 0.8          # a 1.3x straggler scores ~0.77 (> the 0.75 default)
C2 = dict(R=64, K=2048, s_push=10000, cap=8192)
C3 = dict(R=4096, K=2048, s_push=1024, cap=8192)
C4 = dict(R=16384, K=2048, cap=8192)
RECORD_BYTES = 8  # {u32 slot, u32 ns}
STATS_BYTES_PER_SEGMENT = 24  # num/min/max/med/avg/std written per segment


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def launch_ranks(nproc: int) -> int:
    """Start `torch.distributed.run` with nproc ranks of this script as a child process (no
    exec: nothing in this process has touched the GPU, and it only waits) and return its exit
    status.  Rendezvous on 127.0.0.1 with a free port."""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    log("launching:", " ".join(cmd))
    return subprocess.call(cmd)


def dist_setup(dry_run=False):
    """One process per GPU over RCCL.  NVRX_BENCH_BACKEND=gloo is a rehearsal mode only:
    every rank on GPU (LOCAL_RANK mod the visible GPUs), partials exchanged over gloo --
    the multi-rank code path of this script on a one-GPU box; never a reported number."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("NVRX_BENCH_BACKEND", "nccl")
    if dry_run:  # rendezvous only, on the CPU
        if world > 1:
            torch.distributed.init_process_group("gloo")
        return rank, world, torch.device("cpu")
    if backend == "gloo":
        local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    if world > 1:
        if backend == "gloo":
            torch.distributed.init_process_group("gloo")
        else:
            torch.distributed.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"))
    return rank, world, torch.device(f"cuda:{local}")


def allreduce(x: float, op, world, dev) -> float:
    if world == 1:
        return x
    gloo = torch.distributed.get_backend() == torch.distributed.Backend.GLOO
    t = torch.tensor([x], dtype=torch.float64, device="cpu" if gloo else dev)
    torch.distributed.all_reduce(t, op=op)
    return float(t.item())


def barrier(world):
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()


def make_shard(R, K_global, s_push, world, rank, dev, seed=synth.SEED):
    """This rank's kernels of a [R][K_global][s_push] matrix.  seed: the per-sample jitter; the
    straggler ranks stay the default seed's, so every input carries the same straggler set."""
    names = synth.kernel_names(K_global)
    kidx = synth.shard_kernels(names, world, rank) if world > 1 else np.arange(K_global)
    kmap = torch.from_numpy(kidx).to(dev)
    strag = torch.from_numpy(synth.straggler_ranks(R)).to(dev)
    ns = synth.synth_matrix(R, len(kidx), s_push, K_global=K_global, kmap=kmap, straggler=strag,
                            seed=seed, device=dev)
    return ns, kidx


# The pipelined legs give each report in flight its own input (two matrices / record sets that
# differ in every sample): no report can be served by cache lines another report just pulled
# (the reference reads fresh rings every report, straggler.py:237-243)
INPUTS_IN_FLIGHT = 2
SEED_ALT = synth.SEED ^ 0x5A5A5A5A


def on_first_input(pipe):
    """One more (untimed) report at a time until one reads the first input set: the result the
    legs report (straggler sets, the strong-scaled legs' score digest compared across N) is then
    the same input's on every N, whatever the warm-up count was."""
    while True:
        pipe.submit()
        res, _ = pipe.collect()
        if pipe.last_input == 0:
            return res


def timed_pipe_loop(pipe, steps, world, mode="spin"):
    """`steps` back-to-back reports, two in flight, between barriers, with the host waiting in
    the given sync mode (batch.SYNC_MODES).  Returns (last result, elapsed s)."""
    prev = batch.set_sync_mode(mode)
    try:
        barrier(world)
        t0 = time.perf_counter()
        pipe.submit()
        res = None
        for i in range(steps):
            if i + 1 < steps:
                pipe.submit()
            res, _ = pipe.collect()
        barrier(world)
        return res, time.perf_counter() - t0
    finally:
        batch.set_sync_mode(prev)


TIMED_REPORTS = 10  # statistics-kernel timing phase after the throughput loop
TIMED_REPS = 4      # statistics phases back to back in one graph per timed report (events around it)
# Untimed warm-up runs at least `warmup` reports AND at least this long: MI355X clocks ramp under
# sustained load, and a timed run that starts after a few milliseconds of work reads ~3 % slower
# per report at 20 reports (profiles/r04/pipeline_fill.json)
WARMUP_MIN_MS = 40.0


def warm(step, n_min: int, world: int) -> int:
    """step() at least n_min times and, on one rank, until WARMUP_MIN_MS elapsed (on N ranks a
    step may hold a collective, so every rank runs the same count: n_min); returns the count."""
    t0, n = time.perf_counter(), 0
    while n < n_min or (world == 1 and (time.perf_counter() - t0) * 1e3 < WARMUP_MIN_MS):
        step()
        n += 1
    return n


def warm_pipelined(pipe, warmup: int, world: int) -> int:
    """The untimed warm-up of a pipelined loop in its own pattern (two reports in flight, report
    i+1 queued before report i is collected), at least `warmup` reports and WARMUP_MIN_MS (warm());
    drained at the end, so the timed region starts from an empty pipeline."""
    pipe.submit()

    def one():
        pipe.submit()
        pipe.collect()
    n = warm(one, max(1, warmup), world)
    pipe.collect()
    return n


def phases_loop(rep, ns, s_push, g, steps, world, time_kernel):
    """One report at a time: per report the statistics phase (a HIP graph, or eager without
    one) between two timing events, then the rest -- on N GPUs the shard's score partials, the
    eager all_gather and the combine; on 1 GPU the scores graph.  Returns (last result, elapsed
    s between barriers, mean statistics ms or None)."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(steps)]
    res = None
    barrier(world)
    t0 = time.perf_counter()
    for i in range(steps):
        if time_kernel:
            ev[i][0].record()
        if g is not None:
            g.run_stats()
        else:
            rep.compute_stats(ns, s_push)
        if time_kernel:
            ev[i][1].record()
        if g is not None:
            res = g.run_rest()
        else:
            rep.compute_scores()
            res = rep.land()
    barrier(world)
    elapsed = time.perf_counter() - t0
    kern_ms = float(np.mean([a.elapsed_time(b) for a, b in ev])) if time_kernel else None
    return res, elapsed, kern_ms


def phases_label(rep, g) -> str:
    return ("eager" if g is None else
            "hip_graph: statistics | score partials | eager all_gather | combine" if rep.exchange else
            "hip_graph: statistics | rest")


def run_config(cfg, K_global, steps, warmup, world, rank, dev, time_kernel=True, use_graph=True,
               graph_phases=False, lean=False):
    """Full reports on one configuration.  use_graph: every report replays HIP graphs of the
    same kernels (one graph launch instead of one host launch per operation) -- on 1 GPU two
    whole-report graphs in flight (MatrixReporter.pipelined), on N GPUs the stats graph, the
    eager partials exchange, then the rest; the stats phase is timed with HIP events.
    lean: the warm-up and the timed loop only (no bounded-wait loop, no statistics-kernel
    timing, no graph phases).  "res_last" is the result of the timed loop's last report."""
    if lean:
        time_kernel = graph_phases = False
    R, s_push, cap = cfg["R"], cfg["s_push"], cfg["cap"]
    ns, kidx = make_shard(R, K_global, s_push, world, rank, dev)
    K_local = len(kidx)
    rep = batch.MatrixReporter(R, K_local, cap=cap, thr_rel=THR, thr_ind=THR, device=dev)
    for _ in range(warmup):
        res = rep.report(ns, s_push)
    if use_graph:
        # reports two in flight (batch.PipelinedReports), each on its own stream -- report i+1 is
        # queued before report i's results are read on the host; every report lands (host
        # unpack of the results written to pinned memory) inside the timed region, which holds
        # nothing but back-to-back reports.  N GPUs: per report statistics, the shard's partials
        # and the combine as graphs, the all_gather of the partials eager between them
        ns_alt, _ = make_shard(R, K_global, s_push, world, rank, dev, seed=SEED_ALT)
        pipe = rep.pipelined([ns, ns_alt], s_push, timing=time_kernel, timing_reps=TIMED_REPS)
        warm_pipelined(pipe, warmup, world)
        # the warm-up's report count depends on the clock (WARMUP_MIN_MS): one more untimed
        # report where needed, so that the timed loop starts on the first input set on every run
        # and its last report reads the same input whenever the arguments are the same
        while pipe.n % pipe.depth:
            pipe.submit()
            pipe.collect()
        res, elapsed = timed_pipe_loop(pipe, steps, world, "spin")
        res_last = res
        keep = min(s_push, cap)
        if lean:
            label = pipe_label(pipe)
            del ns_alt, pipe
            return dict(ns=ns, kidx=kidx, rep=rep, res=res, res_last=res_last, elapsed=elapsed,
                        kern_ms=None, samples=R * K_local * keep, nseg=R * K_local, keep=keep,
                        launch=label, phases=None)
        # the same loop with the API's default host wait (bounded spin, then block)
        res_b, elapsed_bounded = timed_pipe_loop(pipe, steps, world, "bounded")
        # the roofline's kernel time: after the throughput loop, same process and buffers,
        # reports submitted on an idle device with HIP events around the statistics phase
        ks = []
        if time_kernel:
            # host waits poll here too: a host just woken from a blocking wait queues the graph
            # after the pre-roll spin has ended, and the first event would time that gap
            prev = batch.set_sync_mode("spin")
            for _ in range(TIMED_REPORTS):
                pipe.submit(timed=True)
                res_t, ms = pipe.collect()
                ks.append(ms)
            batch.set_sync_mode(prev)
            barrier(world)
        res = on_first_input(pipe)
        phases = None
        if graph_phases:
            # one report at a time (statistics graph between timing events, then the rest; N
            # GPUs: partials | eager all_gather | combine), same reporter, buffers and warm-up
            # rule, on every N: a 1 -> N curve of either field compares one launch mode
            g = rep.graph(ns, s_push)
            warm(g.run, max(1, warmup), world)
            prev = batch.set_sync_mode("spin")
            res_p, el_p, km_p = phases_loop(rep, ns, s_push, g, steps, world, time_kernel)
            batch.set_sync_mode("bounded")
            _, el_pb, _ = phases_loop(rep, ns, s_push, g, steps, world, False)
            batch.set_sync_mode(prev)
            phases = dict(elapsed=el_p, elapsed_bounded=el_pb, kern_ms=km_p,
                          launch=phases_label(rep, g), sets=res_p.stragglers_relative)
        label = pipe_label(pipe)
        del ns_alt, pipe
        return dict(ns=ns, kidx=kidx, rep=rep, res=res, res_last=res_last, elapsed=elapsed,
                    elapsed_bounded=elapsed_bounded,
                    sets_bounded_ok=bool(np.array_equal(res_b.stragglers_relative, res.stragglers_relative)),
                    kern_ms=float(np.mean(ks)) if ks else None,
                    samples=R * K_local * keep, nseg=R * K_local, keep=keep,
                    launch=label, phases=phases)
    # eager launches (--no-graph), one report at a time
    res, elapsed, kern_ms = phases_loop(rep, ns, s_push, None, steps, world, time_kernel)
    keep = min(s_push, cap)
    launch = phases_label(rep, None)
    return dict(ns=ns, kidx=kidx, rep=rep, res=res, res_last=res, elapsed=elapsed, kern_ms=kern_ms,
                samples=R * K_local * keep, nseg=R * K_local, keep=keep, launch=launch,
                phases=None if lean else dict(elapsed=elapsed, kern_ms=kern_ms, launch=launch,
                                              sets=res.stragglers_relative))


def score_digest(res) -> dict:
    """Order-independent digest of a report's scores (NaN-free sums, f64): a strong-scaled leg's
    digest on N ranks equals the single-GPU one up to the f64 rounding of the shard combine."""
    return dict(rel_sum=float(np.nansum(res.gpu_relative)), ind_sum=float(np.nansum(res.gpu_individual)),
                stragglers_rel=[int(i) for i in np.nonzero(res.stragglers_relative)[0]])


def dump_outputs(path: str, res) -> None:
    """--dump-outputs: a report's results as a caller receives them (batch.BatchResult), one
    <field>.npy each -- the f64 scores as they are, the straggler masks and the error word as
    float32."""
    os.makedirs(path, exist_ok=True)
    for name, a, dt in (("gpu_relative", res.gpu_relative, np.float64),
                        ("gpu_individual", res.gpu_individual, np.float64),
                        ("stragglers_relative", res.stragglers_relative, np.float32),
                        ("stragglers_individual", res.stragglers_individual, np.float32),
                        ("err", [res.err], np.float32)):
        if a is not None:
            np.save(os.path.join(path, name + ".npy"), np.asarray(a, dtype=dt))


def gather_labels(label: str, world: int):
    """Every rank's label (its launch mode), rank order."""
    if world == 1:
        return [label]
    out = [None] * world
    torch.distributed.all_gather_object(out, label)
    return out


def pipe_label(pipe) -> str:
    """The launch label of a batch.PipelinedReports loop (its mode: alt / side / whole)."""
    base = {"alt": "hip_graph: reports two in flight, each on its own stream",
            "side": "hip_graph: reports two in flight, statistics | rest on two streams",
            "whole": "hip_graph: whole reports, two in flight"}[pipe.mode]
    if pipe.rep.exchange:
        base += " (statistics | score partials | eager all_gather | combine)"
    return base


def run_zipf(steps, warmup, world, rank, dev, cpu_ranks, threads):
    """configs[3]: record streams of R ranks (kernels sharded by name hash over N GPUs, the
    whole R on every GPU), one full report per step."""
    R, K, cap = C4["R"], C4["K"], C4["cap"]
    counts = synth.zipf_counts(K)
    slot, occ = synth.zipf_order(counts)
    names = synth.kernel_names(K)
    kidx = synth.shard_kernels(names, world, rank) if world > 1 else np.arange(K)
    lslot, kglob, locc = synth.shard_order(slot, occ, kidx)
    N = lslot.size
    t = lambda a: torch.from_numpy(a.view(np.int32)).to(dev)
    recs = synth.synth_records(R, t(lslot), t(locc), K, int(counts.max()), kglob=t(kglob))
    recs_alt = synth.synth_records(R, t(lslot), t(locc), K, int(counts.max()), kglob=t(kglob),
                                   straggler=torch.from_numpy(synth.straggler_ranks(R)).to(dev),
                                   seed=SEED_ALT)
    rec_off = torch.arange(R + 1, dtype=torch.int64, device=dev) * N
    rep = batch.MatrixReporter(R, len(kidx), cap=cap, thr_rel=THR, thr_ind=THR, device=dev)
    for _ in range(warmup):
        res = rep.report_records(recs, rec_off)
    # reports two in flight on two streams, each on its own record set, as the headline
    # (MatrixReporter.pipelined_records; N GPUs: statistics, partials and combine as graphs, the
    # all_gather eager between them); the statistics phase timed afterwards on an idle device
    pipe = rep.pipelined_records([recs, recs_alt], rec_off, timing=True, timing_reps=TIMED_REPS)
    warm_pipelined(pipe, warmup, world)
    res, elapsed = timed_pipe_loop(pipe, steps, world, "spin")
    ks = []
    prev = batch.set_sync_mode("spin")  # as run_config's timed reports
    for _ in range(TIMED_REPORTS):
        pipe.submit(timed=True)
        ks.append(pipe.collect()[1])
    batch.set_sync_mode(prev)
    res = on_first_input(pipe)
    stats_ms = comm_max(float(np.mean(ks)), world, dev)
    launch = pipe_label(pipe)
    tmax = allreduce(elapsed, torch.distributed.ReduceOp.MAX if world > 1 else None, world, dev)
    nrec = allreduce(float(R * N), torch.distributed.ReduceOp.SUM if world > 1 else None, world, dev)
    out = dict(ranks=R, kernels=K, records_per_rank=int(counts.sum()), cap=cap,
               launch_per_rank=gather_labels(launch, world), scores=score_digest(res),
               ms_per_report=tmax / steps * 1e3, records_per_s=nrec * steps / tmax,
               bucket_plus_stats_ms=stats_ms,
               hbm_frac_of_report=R * N * RECORD_BYTES / (tmax / steps) / HBM_PEAK,
               hbm_frac_of_stats=R * N * RECORD_BYTES / (stats_ms * 1e-3) / HBM_PEAK,
               alg_bytes_per_record=RECORD_BYTES, steps=steps, inputs_in_flight=INPUTS_IN_FLIGHT,
               # HBM bytes per record the bucketing + class kernels move (committed rocprofv3
               # --pmc passes, FETCH_SIZE x2) and the floor of any bucket-then-reduce design:
               # read 8 B, write the kept 4 B payload, read it back
               traffic_bytes_per_record=zipf_pmc_traffic(),
               design_floor_bytes_per_record=16,
               kernels_per_rank=shard_sizes(K, world),
               straggler_sets_exact=all_ranks(bool(np.array_equal(
                   res.stragglers_relative, synth.straggler_ranks(R).astype(bool))), world, dev))
    if world == 1 and rank == 0 and cpu_ranks > 0:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle as O
        h = recs[:cpu_ranks * N].cpu().numpy().view(np.uint32)
        off = np.arange(cpu_ranks + 1, dtype=np.int64) * N
        t1 = time.perf_counter()
        st = O.records_stats(h, off, K, cap=cap, nthreads=threads, route="baseline")
        gr, gi = O.scores(st["num"].reshape(cpu_ranks, K), st["med"].reshape(cpu_ranks, K),
                          st["avg"].reshape(cpu_ranks, K))
        O.stragglers(gr, THR)
        dt = time.perf_counter() - t1
        g = rep.stats
        n = cpu_ranks * K
        parity = all(np.array_equal(getattr(g, f)[:n].cpu().numpy().view(np.int32), st[f].view(np.int32))
                     for f in ("num", "min", "max", "med"))
        out["cpu_baseline"] = dict(value=cpu_ranks * N / dt, unit="records/s", cores=threads,
                                   kind="port", sample=f"{cpu_ranks} of {R} ranks ({cpu_ranks * N} "
                                   f"records, {dt:.2f} s): per-record ring pushes + std::sort "
                                   f"computeStats (oracle/baseline.cpp) + scoring restatement",
                                   gpu_stats_bit_exact_on_sample=parity)
    return out


def run_dropin_api(dev, n_reports=50, K=2048, nsec=3):
    """The drop-in API itself at K = 2048 kernels: one rank's ReportGenerator.generate_report
    (reporting.py:421-554) on the summaries a Detector hands over -- what a training job pays per
    report per process.  Against it: the same inputs through the CPU Python restatement of the
    reference's ReportGenerator (oracle/oracle_report.py, timed the same way) and the reference
    itself, 13.6 ms per report at ws = 1, K = 2048 in the survey container."""
    from nvidia_resiliency_ext.straggler import Statistic, reporting
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_report as OR

    rng = np.random.default_rng(7)
    names = synth.kernel_names(K)
    num = rng.integers(1, 8193, K)
    med = (rng.integers(2_000, 2_000_000, K) / np.float32(1000.0)).astype(np.float32)
    avg = (med * np.float32(1.02)).astype(np.float32)
    smed = rng.uniform(5.0, 50.0, nsec)

    def summaries(keys, jitter):
        kk = {n: {keys["MIN"]: float(m * 0.9), keys["MAX"]: float(m * 1.2), keys["MED"]: float(m * jitter),
                  keys["AVG"]: float(a * jitter), keys["STD"]: float(m * 0.05), keys["NUM"]: int(c)}
              for n, m, a, c in zip(names, med, avg, num)}
        ss = {f"section_{i}": {keys["MIN"]: m * 0.9, keys["MAX"]: m * 1.1, keys["MED"]: m * jitter,
                               keys["AVG"]: m * jitter, keys["STD"]: 0.1, keys["NUM"]: 100}
              for i, m in enumerate(smed)}
        return ss, kk

    enum_keys = {k: getattr(Statistic, k) for k in ("MIN", "MAX", "MED", "AVG", "STD", "NUM")}
    str_keys = {k: k for k in enum_keys}
    jit = [1.0 + 0.01 * (i % 7) for i in range(n_reports + 1)]
    gpu_in = [summaries(enum_keys, j) for j in jit]
    cpu_in = [summaries(str_keys, j) for j in jit]
    scores = ["relative_perf_scores", "individual_perf_scores"]
    gen = reporting.ReportGenerator(scores_to_compute=scores, gather_on_rank0=True)
    sim = OR.SimWorld(1, scores, gather_on_rank0=True)
    t0 = time.perf_counter()
    gen.generate_report(*gpu_in[0])  # the first report assigns the name ids
    first_ms = (time.perf_counter() - t0) * 1e3
    sim.generate_report([cpu_in[0][0]], [cpu_in[0][1]])
    t0 = time.perf_counter()
    for ss, kk in gpu_in[1:]:
        rep = gen.generate_report(ss, kk)
    gpu_ms = (time.perf_counter() - t0) / n_reports * 1e3
    t0 = time.perf_counter()
    for ss, kk in cpu_in[1:]:
        want = sim.generate_report([ss], [kk])[0]
    cpu_ms = (time.perf_counter() - t0) / n_reports * 1e3
    match = all(abs(getattr(rep, f)[0] - want[f][0]) <= 1e-6 * abs(want[f][0])  # (f32-rounded)
                for f in ("gpu_relative_perf_scores", "gpu_individual_perf_scores"))
    return dict(kernels=K, sections=nsec, world_size=1, reports=n_reports,
                gpu_ms_per_report=gpu_ms, first_report_ms=first_ms,
                report_elapsed_field_ms=rep.generate_report_elapsed_time,
                cpu_python_restatement_ms_per_report=cpu_ms,
                reference_survey_ms_per_report=13.6, scores_match_restatement=match)


def cpu_threads() -> int:
    """Host threads for the CPU baseline: the box's CPU share (OMP_NUM_THREADS, 16 on the GPU
    boxes), never more than this process may run on."""
    t = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or len(os.sched_getaffinity(0))
    return max(1, min(t, len(os.sched_getaffinity(0))))


def comm_max(x: float, world: int, dev) -> float:
    return allreduce(x, torch.distributed.ReduceOp.MAX if world > 1 else None, world, dev)


def all_ranks(flag: bool, world: int, dev) -> bool:
    """True iff the flag holds on every rank (MIN over ranks)."""
    return bool(allreduce(1.0 if flag else 0.0, torch.distributed.ReduceOp.MIN if world > 1 else None,
                          world, dev) > 0.5)


def shard_sizes(K_global: int, world: int):
    """Kernels per rank under hash(name) % world (synth.shard_kernels), for every rank."""
    if world == 1:
        return [K_global]
    names = synth.kernel_names(K_global)
    return [int(synth.shard_kernels(names, world, r).size) for r in range(world)]


def pmc_traffic(workload: str):
    """HBM bytes per launch of the stats kernel from a committed rocprofv3 --pmc summary
    (profiles/pmc_<workload>.json, corrected per MI355X_MICROARCH.md: FETCH_SIZE x2)."""
    p = os.path.join(ROOT, "profiles", f"pmc_{workload}.json")
    if not os.path.exists(p):
        return None
    try:
        with open(p) as f:
            return float(json.load(f)["hbm_bytes_per_launch"])
    except Exception:
        return None


def zipf_pmc_traffic():
    """HBM bytes per record of the configs[3] statistics phase from the committed --pmc passes
    (profiles/pmc_zipf_bucket.json + pmc_zipf_stats.json), or None."""
    tot = 0.0
    for part in ("bucket", "stats"):
        p = os.path.join(ROOT, "profiles", f"pmc_zipf_{part}.json")
        try:
            with open(p) as f:
                tot += float(json.load(f)["total"]["bytes_per_record"])
        except Exception:
            return None
    return tot


def cpu_baseline(ns, kidx, cfg, res_gpu_stats, sample_ranks, threads):
    """Host-CPU Reporter on the first `sample_ranks` ranks of the same workload, threaded over
    `threads` host cores: the reference's per-kernel path restated in C++ (oracle/baseline.cpp:
    every pushed duration through a ring of the last cap, then computeStats with std::sort --
    within a few % of the reference's own code compiled from its sources, per core,
    profiles/r02/cpu_baseline_validation.json) + the C restatement of the scoring.  Also
    checks the GPU stats of those ranks bit for bit."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O

    R, s_push, cap = sample_ranks, cfg["s_push"], cfg["cap"]
    K = len(kidx)
    host = ns[:R].contiguous().cpu().numpy().view(np.uint32).reshape(-1)
    t0 = time.perf_counter()
    st = O.matrix_stats(host, R * K, s_push, 0, s_push, cap, nthreads=threads, route="baseline")
    num = st["num"].reshape(R, K)
    med = st["med"].reshape(R, K)
    avg = st["avg"].reshape(R, K)
    gr, gi = O.scores(num, med, avg)
    O.stragglers(gr, THR)
    dt = time.perf_counter() - t0
    keep = min(s_push, cap)
    g = res_gpu_stats
    n = R * K
    parity = all(
        np.array_equal(getattr(g, f)[:n].cpu().numpy().view(np.uint32 if f != "num" else np.int32),
                       st[f].view(np.uint32 if f != "num" else np.int32))
        for f in ("num", "min", "max", "med"))
    return dict(value=R * K * keep / dt, seconds=dt, samples=R * K * keep, parity=parity)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-latency4096", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample-ranks", type=int, default=16)
    ap.add_argument("--cpu4096-ranks", type=int, default=128)
    ap.add_argument("--no-zipf", action="store_true")
    ap.add_argument("--zipf-cpu-ranks", type=int, default=1024)
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of HIP graph replay")
    ap.add_argument("--dry-run", action="store_true", help="launcher + rendezvous only (no GPU)")
    ap.add_argument("--full", action="store_true",
                    help="also everything beyond the headline figure: bounded-wait loop, roofline, "
                         "graph phases, the 4096-rank and Zipf legs, CPU baselines, drop-in API")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the last timed step's results (what a caller of the report "
                         "receives) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus))
    rank, world, dev = dist_setup(args.dry_run)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE {world}")
    backend = torch.distributed.get_backend() if world > 1 else None
    if args.dry_run:
        if world > 1:
            torch.distributed.barrier()
        if rank == 0:
            print(json.dumps({"dry_run": True, "n_gpus": world, "world_size": world,
                              "backend": backend}), flush=True)
        if world > 1:
            torch.distributed.destroy_process_group()
        return

    # ---------------- value: configs[1] per GPU, kernel-hash sharded (weak) ----------
    K_global = C2["K"] * world
    r = run_config(C2, K_global, args.steps, args.warmup, world, rank, dev, use_graph=not args.no_graph,
                   graph_phases=not args.no_graph, lean=not args.full)
    if args.dump_outputs and rank == 0:  # (after the combine every rank holds the same results)
        dump_outputs(args.dump_outputs, r["res_last"])
    tmax = allreduce(r["elapsed"], torch.distributed.ReduceOp.MAX if world > 1 else None, world, dev)
    total_samples = allreduce(float(r["samples"]), torch.distributed.ReduceOp.SUM if world > 1 else None,
                              world, dev)
    value = total_samples * args.steps / tmax
    ms_per_step = tmax / args.steps * 1e3
    res = r["res"]
    strag_true = synth.straggler_ranks(C2["R"])
    sets_ok = all_ranks(bool(np.array_equal(res.stragglers_relative, strag_true.astype(bool))),
                        world, dev)
    # what the process group itself reports (not the launcher's --gpus)
    world_reported = (torch.distributed.get_world_size()
                      if torch.distributed.is_available() and torch.distributed.is_initialized() else 1)
    launch_per_rank = gather_labels(r["launch"], world)
    line = {
        "metric": "duration samples/s reduced to perf scores; report latency at 4096 ranks",
        "value": value,
        "unit": "samples/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup, "warmup_min_ms": WARMUP_MIN_MS,
        "ms_per_step": ms_per_step,
        # the timed loop's host waits poll (batch.set_sync_mode("spin"))
        "host_wait": "spin", "inputs_in_flight": INPUTS_IN_FLIGHT,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u32",
        "data": "synthetic",
        "config": {"workload": "configs[1]: 64 simulated ranks x 2048 kernels/GPU x 10000 "
                               "int-ns samples pushed (last 8192 kept), full stats + rel/indiv "
                               "scores + straggler sets (thr 0.8)",
                   "ranks": C2["R"], "kernels_per_gpu": C2["K"], "kernels_total": K_global,
                   "samples_pushed": C2["s_push"], "ring_cap": C2["cap"],
                   "parallelism": f"kernel-hash shards x{world}" if world > 1 else "1 GPU",
                   "world_size": world, "world_size_reported": world_reported,
                   "kernels_per_rank": shard_sizes(K_global, world),
                   "backend": backend or "none (1 GPU)",
                   "stats_mode": "fast", "launch": r["launch"], "launch_per_rank": launch_per_rank,
                   "inputs_in_flight": INPUTS_IN_FLIGHT},
        "straggler_sets_exact": sets_ok,
    }
    if not args.full:
        # a plain run: the headline figure only (everything below takes runs of its own)
        if rank == 0:
            print(json.dumps(line), flush=True)
        if world > 1:
            torch.distributed.destroy_process_group()
        return
    # roofline of the dominant kernel (segment stats) on this GPU
    alg_bytes = 4 * r["samples"] + STATS_BYTES_PER_SEGMENT * r["nseg"]
    kern_ms = comm_max(r["kern_ms"], world, dev)  # the slowest rank's stats kernel
    achieved = alg_bytes / (kern_ms * 1e-3)
    sec_steps = max(10, args.steps // 2)  # the configs[2] / configs[3] legs
    # the same workload one report at a time (graph phases), measured after the timed loop
    ph = r["phases"]
    phases = None
    if ph is not None:
        tph = comm_max(ph["elapsed"], world, dev)
        phases = dict(ms_per_step=tph / args.steps * 1e3, value=total_samples * args.steps / tph,
                      launch=ph["launch"], launch_per_rank=gather_labels(ph["launch"], world),
                      stats_kernel_ms=comm_max(ph["kern_ms"], world, dev) if ph["kern_ms"] else None,
                      straggler_sets_exact=all_ranks(bool(np.array_equal(
                          ph["sets"], synth.straggler_ranks(C2["R"]).astype(bool))), world, dev))

    # ---------------- secondary: report latency at 4096 ranks (strong) ---------------
    lat = None
    if not args.no_latency4096:
        del r["ns"]
        torch.cuda.empty_cache()
        r4 = run_config(C3, C3["K"], sec_steps, 3, world, rank, dev, time_kernel=True,
                        use_graph=not args.no_graph, graph_phases=not args.no_graph)
        t4 = allreduce(r4["elapsed"], torch.distributed.ReduceOp.MAX if world > 1 else None, world, dev)
        tot4 = allreduce(float(r4["samples"]), torch.distributed.ReduceOp.SUM if world > 1 else None,
                         world, dev)
        n4 = sec_steps
        s4 = r4["res"]
        k4 = comm_max(r4["kern_ms"], world, dev)
        lat = dict(ranks=C3["R"], kernels=C3["K"], samples_per_kernel=C3["s_push"],
                   launch_per_rank=gather_labels(r4["launch"], world), scores=score_digest(s4),
                   ms_per_report=t4 / n4 * 1e3, samples_per_s=tot4 * n4 / t4,
                   stats_kernel_ms=k4,
                   stats_kernel_hbm_frac=(4 * r4["samples"] + 24 * r4["nseg"]) / (k4 * 1e-3) / HBM_PEAK,
                   # one report at a time (samples resident -> scores + sets on the host): the
                   # latency itself; ms_per_report above is the pipelined rate
                   latency_ms_one_report=(comm_max(r4["phases"]["elapsed"], world, dev) / n4 * 1e3
                                          if r4.get("phases") else None),
                   # the same two with the batch API's default host wait (bounded spin, then block)
                   ms_per_report_bounded_wait=(comm_max(r4["elapsed_bounded"], world, dev) / n4 * 1e3
                                               if r4.get("elapsed_bounded") is not None else None),
                   latency_ms_one_report_bounded_wait=(
                       comm_max(r4["phases"]["elapsed_bounded"], world, dev) / n4 * 1e3
                       if r4.get("phases") and "elapsed_bounded" in r4["phases"] else None),
                   inputs_in_flight=INPUTS_IN_FLIGHT,
                   steps=n4, kernels_per_rank=shard_sizes(C3["K"], world),
                   straggler_sets_exact=all_ranks(bool(np.array_equal(
                       s4.stragglers_relative, synth.straggler_ranks(C3["R"]).astype(bool))), world, dev))
        if world == 1 and rank == 0 and not args.no_cpu_baseline:
            # the north_star's >= 100x target is stated at this configuration
            cb4 = cpu_baseline(r4["ns"], r4["kidx"], C3, r4["rep"].stats, args.cpu4096_ranks,
                               cpu_threads())
            lat["cpu_baseline"] = dict(
                value=cb4["value"], unit="samples/s", cores=cpu_threads(), kind="port",
                per_core=cb4["value"] / cpu_threads(),
                sample=f"{args.cpu4096_ranks} of 4096 ranks x 2048 kernels x 1024 samples "
                       f"({cb4['samples']:.3g} samples, {cb4['seconds']:.2f} s): ring pushes + "
                       f"std::sort computeStats (oracle/baseline.cpp) + scoring restatement",
                gpu_stats_bit_exact_on_sample=cb4["parity"],
                cpu_report_ms_extrapolated=4096 * 2048 * 1024 / cb4["value"] * 1e3)
            lat["gpu_over_cpu"] = lat["samples_per_s"] / cb4["value"]
        del r4
        torch.cuda.empty_cache()

    threads = cpu_threads()
    # ---------------- configs[3]: Zipf record streams at 16k ranks --------------------
    zipf = None
    if not args.no_zipf:
        torch.cuda.empty_cache()
        zipf = run_zipf(sec_steps, 3, world, rank, dev,
                        0 if args.no_cpu_baseline else args.zipf_cpu_ranks, threads)
        torch.cuda.empty_cache()

    # ---------------- configs[0] shape: a small world's report latency (rank 0, N == 1) ----
    # 8 ranks x 200 kernels x 1000 samples (the reference's CPU/gloo case, BASELINE.md: 29.1 ms
    # per report in the survey container): the whole HIP report vs the CPU restatement
    # (computeStats + scoring) on the same inputs
    c1 = None
    if world == 1 and rank == 0 and not args.no_cpu_baseline:
        C1 = dict(R=8, K=200, s_push=1000, cap=8192)
        n1 = 50
        r1 = run_config(C1, C1["K"], n1, 5, 1, 0, dev, time_kernel=False, use_graph=not args.no_graph)
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle as O
        host = r1["ns"].contiguous().cpu().numpy().view(np.uint32).reshape(-1)
        t1 = time.perf_counter()
        reps1 = 20
        for _ in range(reps1):
            st1 = O.matrix_stats(host, C1["R"] * C1["K"], C1["s_push"], 0, C1["s_push"], C1["cap"],
                                 nthreads=min(8, threads), route="baseline")
            gr1, _ = O.scores(st1["num"].reshape(C1["R"], C1["K"]), st1["med"].reshape(C1["R"], C1["K"]),
                              st1["avg"].reshape(C1["R"], C1["K"]))
            O.stragglers(gr1, THR)
        cpu_ms = (time.perf_counter() - t1) / reps1 * 1e3
        c1 = dict(ranks=C1["R"], kernels=C1["K"], samples_per_kernel=C1["s_push"],
                  gpu_ms_per_report=r1["elapsed"] / n1 * 1e3,
                  cpu_port_ms_per_report=cpu_ms, cpu_port_cores=min(8, threads),
                  reference_survey_ms_per_report=29.1,
                  gpu_relative_matches_cpu=bool(np.allclose(r1["res"].gpu_relative, gr1, rtol=1e-6)))
        del r1

    # ---------------- the drop-in ReportGenerator at 2048 kernels (rank 0, N == 1) -------
    api = run_dropin_api(dev) if world == 1 and rank == 0 and not args.no_cpu_baseline else None

    # ---------------- CPU baseline (rank 0, N == 1 only) ------------------------------
    cpu = None
    if world == 1 and rank == 0 and not args.no_cpu_baseline:
        ns_c2, kidx = make_shard(C2["R"], C2["K"], C2["s_push"], 1, 0, dev)
        rep = batch.MatrixReporter(C2["R"], len(kidx), cap=C2["cap"], device=dev)
        rep.compute_stats(ns_c2, C2["s_push"])
        cb = cpu_baseline(ns_c2, kidx, C2, rep.stats, args.cpu_sample_ranks, threads)
        cpu = dict(value=cb["value"], unit="samples/s", cores=threads, kind="port",
                   per_core=cb["value"] / threads,
                   sample=f"{args.cpu_sample_ranks} of 64 ranks x 2048 kernels x 10000 pushed "
                          f"(8192 kept; {cb['samples']:.3g} samples, {cb['seconds']:.2f} s): ring "
                          f"pushes + std::sort computeStats (oracle/baseline.cpp) + scoring "
                          f"restatement",
                   gpu_stats_bit_exact_on_sample=cb["parity"])

    # (collectives: on every rank, before rank 0 writes the line)
    ms_bounded = (comm_max(r["elapsed_bounded"], world, dev) / args.steps * 1e3
                  if r.get("elapsed_bounded") is not None else None)
    sets_bounded = (all_ranks(r["sets_bounded_ok"] and sets_ok, world, dev)
                    if "sets_bounded_ok" in r else None)
    if rank == 0:
        # the committed PMC pass is of the 1-GPU launch (64 x 2048 segments); a shard of
        # 2048*N hashed kernels has a different size, so its traffic is not claimed
        traffic = pmc_traffic("c2_segment_stats") if world == 1 else None
        line.update({
            # the one-report-at-a-time launch mode's time per report on the same workload,
            # measured after the pipelined loop on every N (a like-for-like 1 -> N
            # curve reads this field; "graph_phases" holds its label and rate)
            "ms_per_step_graph_phases": phases["ms_per_step"] if phases else None,
            # the batch API's default host waits poll at most 50 us, then block -- the timed
            # loop in that mode:
            "ms_per_step_bounded_wait": ms_bounded,
            "graph_phases": phases,
            "roofline": {"bound": "hbm", "achieved": achieved / 1e9, "peak": HBM_PEAK / 1e9,
                         "unit": "GB/s", "frac": achieved / HBM_PEAK,
                         "traffic": traffic,
                         "kernel": "seg_stats_lean_group_kernel<128> (4 segments per wave)",
                         "kernel_ms": kern_ms,
                         "alg_bytes_per_launch": alg_bytes,
                         # the same bytes over the pipelined loop's time per report (two reports'
                         # statistics kernels overlap at their boundaries)
                         "per_report_frac": alg_bytes / (ms_per_step * 1e-3) / HBM_PEAK,
                         "kernel_ms_is": "the statistics kernel on an idle device after the loop: "
                                         "HIP events on its stream around one graph of 4 back-to-back "
                                         "statistics phases, "
                                         "10 reports, mean per replay; in the loop two reports' "
                                         "kernels overlap at their launch boundaries, so "
                                         "ms_per_step can be below it"},
            "cpu_baseline": cpu,
            "latency_4096_ranks": lat,
            "configs0_report": c1,
            "dropin_report_2048_kernels": api,
            "zipf_16384_ranks": zipf,
            "straggler_sets_exact_bounded_wait": sets_bounded,
        })
        print(json.dumps(line), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
