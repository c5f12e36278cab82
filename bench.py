#!/usr/bin/env python3
"""bench.py -- headline benchmark of the render hot path on MI355X.

Metric (BASELINE.json): Msamples/sec at 4096 partials x 64 voices (one sample = one output frame of
the whole tree, all 64 voice rows), 48 kHz synthetic tree, plus achieved rates against the roofline.

A "step" is one `fill_buffer` call of T = 4800 frames (0.1 s of audio) over the full tree, through the
C ABI's device-resident entry point: the time-ramp input and the output buffer are already in HBM when
the timed region starts.  The timed region is exactly K = --steps steps after W = --warmup untimed ones
(barrier + synchronize on both sides, max over ranks); `ms_per_step` / `value` come from it.  Right before
it a second renderer of the same tree keeps the device busy for DEVICE_WARMUP_S (clock ramp, see run).
`--dump-outputs DIR` writes what the last timed step left in the caller's output buffer (see dump_output).
The reference-shaped host-buffer call (`fr_fill_buffer`: host rows in, host buffer out, synchronous) is
timed separately as `host_api` -- PCIe- and sync-inclusive, never `value`.

N > 1 (launched by torch.distributed.run, one rank per GPU): every rank receives the SAME graph through
the ordinary ABI and `fr_set_shard` makes it rank r of N -- sharding is a property of the engine.
  voices   (default) rank r renders its block of the 64 output rows: strong scaling, no collective.
  partials (default from 16384 partials per voice up: BASELINE configs[4]) every voice's Sum2 tree is cut
           at its top log2(N) levels, rank r renders block r of every voice, one recursive-halving exchange
           over the engine's own RCCL communicator (xGMI) sums the blocks in the tree's own association and
           leaves every rank with the finished voices it owns.  Strong scaling, bit-exact.
  time     an extra: N independent replicas rendering different frames of the same tree (weak scaling).
`value` = frames rendered by the job / max-over-ranks time.

Prints ONE JSON line on stdout (rank 0); diagnostics go to stderr.
"""
import argparse
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# MI355X ceilings (/opt/skills/guides/MI355X_MICROARCH.md: chip-level parameters, cycle constants)
HBM_PEAK_GBS = 8000.0                       # spec; 6290 measured copy
VALU_LANE_RATE = 256 * 4 * 32 * 2.4e9       # f32 VALU lane-ops/s: 256 CUs x 4 SIMD-32 x 2.4 GHz = 78.6e12
OPS_EXECUTED_PER_PF = 6                     # VALU ops the fused kernel issues per partial-frame: mul, fract, fma, fma, mul + 1 tree add
ISSUE_SLOTS_PER_PF = 7                      # v_fract_f32 issues at half rate on gfx950 (measured 4.07 vs 2.2 cyc, profiles/r01_valu_rate.txt)
OPS_GRAPH_PER_PF = 12                       # primitive nodes the reference evaluates per partial-frame (11 + Sum2)
PMC_SUMMARY = os.path.join(ROOT, "profiles", "r03_bank_pmc_summary.json")
DUMP_MAX_BYTES = 64 << 20
DEVICE_WARMUP_S = 0.2                       # seconds of sustained load right before the timed loop (see run)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def dump_output(directory, out):
    """`out` (the [rows, T] f32 buffer a caller of the timed path receives) as <directory>/output.npy.  Above
    DUMP_MAX_BYTES a fixed, seeded sample of its elements is written instead (1-D, row-major order), with their flat
    indices into [rows, T] in output_index.npy (f64, exact), both files together within the limit."""
    os.makedirs(directory, exist_ok=True)
    out = np.ascontiguousarray(out, dtype=np.float32)
    if out.nbytes > DUMP_MAX_BYTES:
        n = (DUMP_MAX_BYTES - 4096) // 12        # 4 B value + 8 B index per element; 4 KiB for the two .npy headers
        idx = np.sort(np.random.default_rng(0).choice(out.size, n, replace=False))
        np.save(os.path.join(directory, "output_index.npy"), idx.astype(np.float64))
        out = out.reshape(-1)[idx]
    np.save(os.path.join(directory, "output.npy"), out)
    log(f"dumped the last timed step's output to {directory}: {out.shape} f32")


def shader_clock_mhz():
    """Current shader clock of the busiest amdgpu card from sysfs (the line marked '*'), or None."""
    best = None
    for path in glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"):
        try:
            for line in open(path):
                if "*" in line:
                    mhz = float(line.split(":")[1].strip().split("M")[0])
                    best = mhz if best is None else max(best, mhz)
        except Exception:
            pass
    return best


def cpu_baseline(tree, V, P, frames_1t, frames_mt):
    """The CPU path, timed on this box's host cores: the C++ restatement of RefRenderer (oracle/, kind
    'port' -- the Rust reference cannot be built here).  Bounded sample of the same workload."""
    from libfriendship_amd import synth
    from libfriendship_amd.capi import Renderer, RendererLib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_tools
    lib = RendererLib(os.path.join(ROOT, "oracle", "_build", "libfr_oracle.so"))
    ncpu = os.cpu_count() or 1
    with Renderer(lib) as r:
        synth.install(r, tree)
        t = synth.time_ramp(0, frames_1t)
        t0 = time.perf_counter()
        out1 = r.fill_buffer(V, 0, frames_1t, [t])
        dt1 = time.perf_counter() - t0
        nthreads = min(ncpu, V)
        oracle_tools.set_threads(r, nthreads)
        t = synth.time_ramp(frames_1t, frames_1t + frames_mt)
        t0 = time.perf_counter()
        r.fill_buffer(V, frames_1t, frames_1t + frames_mt, [t])
        dtm = time.perf_counter() - t0
    one = {"value": frames_1t / dt1 / 1e6, "unit": "Msamples/s", "cores": 1, "kind": "port",
           "sample": f"{frames_1t} frames of the same {P}x{V} tree, single thread (the reference renderer is "
                     f"single-threaded); C++ restatement of RefRenderer, not the Rust binary",
           "seconds": dt1}
    many = {"value": frames_mt / dtm / 1e6, "unit": "Msamples/s", "cores": nthreads, "kind": "port",
            "sample": f"{frames_mt} frames, output slots spread over {nthreads} threads", "seconds": dtm,
            "host_cpus": ncpu}
    return one, many, out1


def other_config(name, torch, libfriendship_amd, synth, device, K, W):
    """One of BASELINE.json's other single-GPU configs as a sub-record of the line (`configs`): configs[1] (B: a 256-partial
    harmonic stack, 1 voice) or configs[3] (D: harmonics + detune + ADSR + 4-tap delay chain, 1024 partials x 128 voices),
    4800-frame calls through the device entry point like the headline: K steps timed after W warm-up steps, the kernels'
    own time from HIP events (fr_set_timing), and parity against the CPU path on sampled (voice, frame) pairs -- the
    evaluator is random-access in time (reference.rs:90-96), so the oracle answers single samples of D from the stored
    input history without rendering the 2^4-fold delay recursion for every frame."""
    from libfriendship_amd.capi import Renderer, RendererLib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_tools
    T = 4800
    if name == "B":
        V, P = 1, 256
        tree = synth.additive_tree(V, P, params_as_nodes=True)
        workload = "BASELINE.json configs[1]: 256-partial harmonic stack, 1 voice, 48 kHz, 4800-frame calls"
    else:
        V, P = 128, 1024
        tree = synth.effects_tree(V, P, params_as_nodes=True)
        workload = "BASELINE.json configs[3]: harmonics + per-partial detune + ADSR envelope + 4-tap delay chain, 1024 partials x 128 voices, 4800-frame calls"
    hip = libfriendship_amd.HipRenderer(device=device)
    synth.install(hip, tree)
    n_calls = W + K + K
    WRAP = 1 << 23
    rows = [(np.arange(k * T, (k + 1) * T, dtype=np.int64) % WRAP).astype(np.float32) for k in range(min(n_calls, 64))]
    d_time = torch.from_numpy(np.concatenate(rows)).cuda()
    d_out = torch.empty((V, T), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    kept = {}

    def step(k):
        row = d_time[(k % len(rows)) * T:][:T]
        hip.fill_buffer_device(d_out.data_ptr(), V, T, k * T, row.data_ptr(), [0, T], stream)

    for k in range(W):
        step(k)
        if k < 8:
            kept[k] = d_out.cpu().numpy().copy()       # (the first calls: compared with the CPU path below)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(W, W + K):
        step(k)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    hip.set_timing(True)
    hip.reset_timing()
    for k in range(W + K, W + 2 * K):
        step(k)
    torch.cuda.synchronize()
    bank_ms, bank_n = hip.get_timing("bank")
    all_ms, all_n = hip.get_timing("all")
    plan = hip.plan()
    hip.set_timing(False)
    hip.close()
    pf = float(V) * P * T
    kern_s = all_ms / K * 1e-3
    rec = {"workload": workload, "voices": V, "partials": P, "frames_per_call": T, "steps": K, "warmup": W,
           "value": K * T / elapsed / 1e6, "unit": "Msamples/s", "ms_per_step": elapsed / K * 1e3,
           "roofline": {"bound": "valu", "unit": "TFLOP/s", "achieved": OPS_EXECUTED_PER_PF * pf / kern_s / 1e12 if kern_s else 0.0,
                        "peak": VALU_LANE_RATE / 1e12, "frac": OPS_EXECUTED_PER_PF * pf / kern_s / VALU_LANE_RATE if kern_s else 0.0,
                        "frac_of_step": OPS_EXECUTED_PER_PF * pf / (elapsed / K) / VALU_LANE_RATE,
                        "kernels_ms_per_step": all_ms / K, "bank_kernel_ms": bank_ms / max(bank_n, 1), "launches_per_step": all_n / K,
                        "note": "oscillator-bank lane-ops (6 per partial-frame) over the time of ALL kernels of a step (bank + stage "
                                "programs), HIP events on the launch stream; frac_of_step: over the step's wall time"},
           "plan": {k: plan.get(k) for k in ("banks", "stage_programs", "fused_programs", "fused_stride", "rings", "max_lookback", "stage_jit", "pull_rows")}}
    # parity on sampled (voice, frame) pairs of the first calls
    try:
        e = tree["edges"]
        oracle = RendererLib(os.path.join(ROOT, "oracle", "_build", "libfr_oracle.so"))
        rng = np.random.default_rng(3)
        n_kept = len(kept)
        with Renderer(oracle) as ref:
            synth.install(ref, dict(tree, edges=e[e[:, 1] != 0]))          # without the output edges: storing the rows renders nothing
            for k in range(n_kept):
                ref.fill_buffer(1, k * T, (k + 1) * T, [rows[k]])
            ref.on_add_edges(e[e[:, 1] == 0])
            voices = np.arange(V) if V <= 8 else np.unique(np.concatenate([[0, V - 1], rng.integers(0, V, 8)]))
            frames = np.unique(np.concatenate([[0, 1, 480, 2400, 2401, T - 1, T, 9600, 12000, 24000, 24001, n_kept * T - 1],
                                               rng.integers(0, n_kept * T, 20 if V == 1 else 6)]))
            frames = frames[frames < n_kept * T]
            t1 = time.perf_counter()
            exp = oracle_tools.eval_samples(ref, np.repeat(voices, len(frames)).astype(np.uint32),
                                            np.tile(frames, len(voices)).astype(np.uint64)).reshape(len(voices), len(frames))
            cpu_s = time.perf_counter() - t1
        got = np.stack([kept[int(f) // T][voices, int(f) % T] for f in frames], axis=1)
        same = (got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp))
        rec["parity"] = {"bit_exact": bool(same.all()), "samples": int(same.size), "voices": int(len(voices)), "frames": int(len(frames)),
                         "frames_span": [0, n_kept * T], "cpu_seconds": cpu_s,
                         "against": "oracle/ref_renderer.cpp (C++ restatement of RefRenderer), random-access samples"}
    except Exception as ex:   # a reported extra; never lose the line over it
        rec["parity"] = {"error": repr(ex)}
    return rec


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n, argv, child_cmd=None, timeout=None):
    """`python bench.py --gpus N` without a launcher around it: this process becomes the launcher.  It starts N children
    of the same command, one rank per GPU (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* as torch.distributed.run would set
    them), forwards rank 0's one JSON line and fails if any rank fails.  The parent never imports torch and never touches
    HIP (a process that has initialised the GPU must not be replaced or forked on this pool): children are fresh
    interpreters.  Returns (exit code, rank 0's last stdout line or None)."""
    import subprocess
    cmd = list(child_cmd) if child_cmd else [sys.executable, os.path.abspath(__file__)]
    port = free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n),
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "FR_BENCH_LAUNCHER": "self"})
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC (RCCL between processes on this driver)
        env.setdefault("OMP_NUM_THREADS", "1")
        # rank 0's stdout carries the line; the others' goes where diagnostics go
        procs.append(subprocess.Popen(cmd + list(argv), env=env, stdout=subprocess.PIPE if r == 0 else sys.stderr,
                                      stderr=sys.stderr, text=(r == 0)))
    t_end = time.monotonic() + timeout if timeout else None
    out0, failed = None, None
    try:
        pending = set(range(n))
        while pending and failed is None:
            for r in sorted(pending):
                rc = procs[r].poll()
                if rc is None:
                    continue
                pending.discard(r)
                if rc != 0:
                    failed = (r, rc)
                    break
            if t_end and time.monotonic() > t_end:
                failed = (-1, 124)
            if pending and failed is None:
                if 0 in pending:     # keep rank 0's pipe drained (one line, but never let it block on a full pipe)
                    try:
                        out0, _ = procs[0].communicate(timeout=0.2)
                        continue
                    except subprocess.TimeoutExpired:
                        pass
                else:
                    time.sleep(0.05)
    finally:
        for p in procs:              # a failed or timed-out job: end exactly the processes started here
            if p.poll() is None:
                p.kill()
        for p in procs:
            try:
                p.wait(timeout=30)
            except Exception:
                pass
    if out0 is None:
        try:
            out0, _ = procs[0].communicate(timeout=30)     # (exited: returns what the pipe still holds, incl. earlier partial reads)
        except Exception:
            out0 = None
    if failed is not None:
        who = "the job timed out" if failed[0] < 0 else f"rank {failed[0]} exited with code {failed[1]}"
        log(f"bench.py launcher: {who}; the other ranks were stopped")
        return (failed[1] if failed[1] else 1), None
    lines = [ln for ln in (out0 or "").splitlines() if ln.strip()]
    return 0, (lines[-1] if lines else None)


def main():
    # `python bench.py --gpus N` with no launcher around it (WORLD_SIZE unset): start the N ranks here, before anything
    # imports torch or touches the GPU.
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--gpus", type=int, default=1)
    pre.add_argument("--launch-timeout", type=float, default=3000.0)
    known, _ = pre.parse_known_args()
    if known.gpus > 1 and "WORLD_SIZE" not in os.environ:
        rc, line = launch_ranks(known.gpus, sys.argv[1:], timeout=known.launch_timeout)
        if rc == 0 and line is None:
            log("bench.py launcher: rank 0 printed no result line")
            rc = 1
        if line is not None:
            sys.stdout.write(line + "\n")
            sys.stdout.flush()
        sys.exit(rc)
    # Exactly ONE line may reach stdout.  Libraries write there too (RCCL prints a version banner at communicator
    # creation), so the process's stdout is pointed at stderr for the whole run and the JSON line goes to the saved
    # descriptor at the end.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    try:
        line = run()
    finally:
        sys.stdout.flush()
        os.dup2(real_stdout, 1)
    if line is not None:
        os.write(real_stdout, (line + "\n").encode())
    os.close(real_stdout)


def run():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed steps (K): the timed region is exactly these K calls")
    ap.add_argument("--warmup", type=int, default=20, help="untimed steps before the timed region (W)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the output of the last timed step (rank 0's rows) as DIR/output.npy; the inputs depend only "
                         "on the arguments, so runs of two builds with the same arguments can be compared")
    ap.add_argument("--voices", type=int, default=64)
    ap.add_argument("--partials", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=4800, help="frames per fill_buffer call (T)")
    ap.add_argument("--mode", default="auto", choices=["auto", "pull"])
    ap.add_argument("--shard", default="auto", choices=["auto", "voices", "partials", "time"],
                    help="how N > 1 ranks split the job (fr_set_shard): voices (strong scaling, no exchange; the default), "
                         "partials (the default from 16384 partials per voice: partial blocks + one RCCL exchange), "
                         "time (an extra: independent replicas on different frames, weak scaling)")
    ap.add_argument("--tree", default="additive", choices=["additive", "effects", "chorus"],
                    help="additive = BASELINE configs[2] shape (the headline); effects = configs[3] shape (detune + ADSR + "
                         "4-tap delay chain), a diagnostic run: use with --voices 128 --partials 1024 --no-cpu-baseline; "
                         "chorus = every voice through a Delay with a SIGNAL amount (LFO) + the 4-tap chain, also a diagnostic")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl is RCCL on ROCm (default): torch.distributed for the barrier and the engine's own RCCL "
                         "communicator for the exchange; gloo = rehearsal on a one-GPU box (exchange through the host callback)")
    ap.add_argument("--force-dist", action="store_true", help="initialise torch.distributed even with one rank (plumbing check)")
    ap.add_argument("--launch-timeout", type=float, default=3000.0,
                    help="--gpus N > 1 without a launcher (WORLD_SIZE unset): bench.py starts its own N ranks; seconds before it gives up on them")
    ap.add_argument("--wrap-voices", type=int, default=0,
                    help="effects tree only, shape sweeps: fundamentals repeat every N voices (synth.voice_params wrap); the "
                         "survey's 55*2^(v/12) puts voices beyond v~150 above any representable pitch (identically zero mixes)")
    ap.add_argument("--streams", type=int, default=1,
                    help="issue consecutive steps round-robin on this many HIP streams (each with its own output buffer): calls "
                         "of a plan without delay state are independent and the engine lets them overlap on the device")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-configs", action="store_true", help="skip the sub-records of BASELINE configs[1] (B) and configs[3] (D)")
    ap.add_argument("--no-extras", action="store_true",
                    help="only the timed workload's kernels (for rocprof runs): no host_api, short_blocks or overlapped_calls legs")
    ap.add_argument("--cpu-frames", type=int, default=144,
                    help="frames the CPU path renders single-threaded for cpu_baseline and the parity check (about 12 s)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    import torch
    import torch.distributed as dist
    import libfriendship_amd
    from libfriendship_amd import synth

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log(f"warning: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE")
    launcher = "none" if world == 1 else ("bench.py (self-spawned ranks)" if os.environ.get("FR_BENCH_LAUNCHER") == "self" else "external (torch.distributed.run)")
    # (rehearsals on a one-GPU box: several ranks may share device 0 with --backend gloo)
    local_rank = local_rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local_rank)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo")

    V, P, T, K, W = args.voices, args.partials, args.frames, args.steps, args.warmup
    shard_mode = args.shard
    if shard_mode == "auto":
        shard_mode = "partials" if P >= 16384 and world > 1 and (world & (world - 1)) == 0 else "voices"
    if world == 1:
        shard_mode = "none"
    t_build = time.perf_counter()
    # Seeded synthetic tree, ~12 primitive nodes per partial plus the harmonics / detune / sample-rate
    # arithmetic as Multiply / Divide nodes over constants (N3, N4: the reference has only the seven primitives).  EVERY
    # rank installs the whole tree: what a rank renders is decided by the engine (fr_set_shard), not by graph surgery.
    if args.tree == "effects":
        tree = synth.effects_tree(V, P, wrap=args.wrap_voices or None, params_as_nodes=True)
    elif args.tree == "chorus":
        tree = synth.chorus_tree(V, P, taps=4)
    else:
        tree = synth.additive_tree(V, P, params_as_nodes=True)
    hip = libfriendship_amd.HipRenderer(mode=args.mode, device=local_rank)
    synth.install(hip, tree)
    log(f"[rank {rank}] graph: {len(tree['handles'])} nodes, {len(tree['edges'])} edges, "
        f"installed in {time.perf_counter() - t_build:.1f}s")

    transport = "none"

    def make_shard(serial_exchange=False):
        """fr_set_shard on every rank (collective with RCCL: a fresh communicator id each time)."""
        nonlocal transport
        if shard_mode == "voices":
            hip.set_shard(rank, world, "voices")     # no exchange in this mode: no transport, no communicator
        elif shard_mode == "partials":
            if args.backend == "nccl":
                # the engine's own communicator: rank 0 draws the id, torch.distributed carries the 128 bytes
                idt = torch.zeros(128, dtype=torch.uint8, device="cuda")
                if rank == 0:
                    idt.copy_(torch.frombuffer(bytearray(libfriendship_amd.hip_lib().comm_unique_id()), dtype=torch.uint8))
                dist.broadcast(idt, 0)
                hip.set_shard(rank, world, shard_mode, rccl_id=bytes(idt.cpu().numpy().tobytes()), serial_exchange=serial_exchange)
                transport = "rccl"
            else:
                def sendrecv(peer, send, recv):   # rehearsal: host buffers over gloo
                    reqs, rt = [], None
                    if send is not None:
                        reqs.append(dist.isend(torch.from_numpy(send.copy()), peer))
                    if recv is not None:
                        rt = torch.empty(recv.size, dtype=torch.uint8)
                        reqs.append(dist.irecv(rt, peer))
                    for q in reqs:
                        q.wait()
                    if recv is not None:
                        recv[:] = rt.numpy()
                hip.set_shard(rank, world, shard_mode, sendrecv=sendrecv, serial_exchange=serial_exchange)
                transport = "host-callback (gloo)"

    if world > 1:
        make_shard()
    row_lo, row_hi = hip.shard_rows(V)

    # Every step's time-ramp row is already resident in HBM.  The ramp is the f32 frame number, exact below 2^24, so
    # its VALUES wrap at 2^23 (idx itself, a u64, keeps counting); rows live in a ring of at most 64 steps.
    stripe0 = rank * (W + 52 * K + 64) * T if shard_mode == "time" else 0     # (more frames than any rank renders)
    ring_steps = min(W + K, 64)
    WRAP = 1 << 23

    def ramp_row(k):
        f0 = stripe0 + k * T
        return (np.arange(f0, f0 + T, dtype=np.int64) % WRAP).astype(np.float32)

    d_time = torch.from_numpy(np.concatenate([ramp_row(k) for k in range(ring_steps)])).cuda()
    d_out = torch.empty((max(V, 1), T), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    n_streams = max(1, args.streams)
    side_streams = [torch.cuda.Stream() for _ in range(n_streams)] if n_streams > 1 else []
    side_outs = [torch.empty_like(d_out) for _ in range(n_streams)] if n_streams > 1 else []

    def step(k):
        row = d_time[(k % ring_steps) * T:][:T]
        if side_streams:
            hip.fill_buffer_device(side_outs[k % n_streams].data_ptr(), V, T, stripe0 + k * T, row.data_ptr(), [0, T],
                                   side_streams[k % n_streams].cuda_stream)
            return
        hip.fill_buffer_device(d_out.data_ptr(), V, T, stripe0 + k * T, row.data_ptr(), [0, T], stream)

    def barrier():
        if use_dist:
            dist.barrier()

    def max_over_ranks(x):
        if not use_dist:
            return x
        te = torch.tensor([x], dtype=torch.float64, device="cuda" if args.backend == "nccl" else "cpu")
        dist.all_reduce(te, op=dist.ReduceOp.MAX)
        return float(te.item())

    t0 = time.perf_counter()
    for k in range(W):           # first call also lowers the graph and uploads the bank parameters
        step(k)
    torch.cuda.synchronize()
    log(f"[rank {rank}] warmup ({W} steps incl. lowering): {time.perf_counter() - t0:.2f}s; plan: {hip.plan()}")

    def timed_loop(k0):
        # barrier + synchronize, K steps, synchronize + barrier; every rank clocks its own K steps (from leaving the opening
        # barrier to its own synchronize) and the job's time is the MAX over ranks -- the closing barrier's own latency
        # (tens of microseconds over RCCL, as much as two steps of a voice-sharded job) is not rendering time
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(k0, k0 + K):
            step(k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        barrier()
        return max_over_ranks(dt)

    # Device warm-up.  The first ~30 ms of sustained load run 5-13% slower than the steady state (clock ramp), and W steps
    # of a tree can take well under a millisecond.  A second renderer of the same tree keeps the device busy with the same
    # calls for DEVICE_WARMUP_S right before the timed region, so the measured renderer itself runs exactly W untimed and
    # K timed steps and what it computes depends only on the arguments.
    warm = libfriendship_amd.HipRenderer(mode=args.mode, device=local_rank)
    synth.install(warm, tree)
    warm_out = torch.empty_like(d_out)

    def warm_step(k):
        warm.fill_buffer_device(warm_out.data_ptr(), V, T, k * T, d_time[(k % ring_steps) * T:][:T].data_ptr(), [0, T], stream)

    warm_step(0)                 # lowering
    torch.cuda.synchronize()
    n_warm, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < DEVICE_WARMUP_S:
        for _ in range(8):
            n_warm += 1
            warm_step(n_warm)
        torch.cuda.synchronize()
    warm_s = time.perf_counter() - t0

    elapsed = timed_loop(W)
    clock = shader_clock_mhz()
    warm.close()
    next_k = W + K
    # what the last timed step left in the buffer its caller reads (the timed loop ended in a device-wide synchronize)
    last = (side_outs[(next_k - 1) % n_streams] if side_streams else d_out).cpu().numpy()
    if args.dump_outputs and rank == 0:
        dump_output(args.dump_outputs, last[row_lo:row_hi])
    # Partial-block sharding: the same steps with the exchange as ONE serial step behind the bank kernels (round 2's form,
    # FR_SHARD_SERIAL_EXCHANGE) beside the time-tiled, overlapped exchange measured above (SURVEY 8e asks for both numbers)
    exchange = None
    if world > 1 and shard_mode == "partials":
        st_tiled = hip.plan().get("exchange_stats", {})
        make_shard(serial_exchange=True)
        for k in range(next_k, next_k + W):
            step(k)
        torch.cuda.synchronize()
        t_serial = [timed_loop(next_k + W + i * K) for i in range(3)]
        st_serial = hip.plan().get("exchange_stats", {})
        next_k += W + 3 * K
        calls_t = max(st_tiled.get("calls", 0), 1)
        exchange = {"overlapped_ms_per_step": elapsed / K * 1e3, "serial_ms_per_step": statistics.median(t_serial) / K * 1e3,
                    "tiles_per_call": st_tiled.get("tiles", 0) / calls_t, "bytes_sent_per_rank_per_step": st_tiled.get("bytes_sent", 0) / calls_t,
                    "transport": transport,
                    "note": ("rehearsal: ranks share one GPU, host buffers over gloo -- not an xGMI number" if args.backend == "gloo" else
                             "engine's own RCCL communicator, pairwise ncclSend/ncclRecv per recursive-halving step") +
                            "; tile i's exchange runs on a second stream under the bank kernels of tile i + 1; same bits either way",
                    "serial_stats": {k: st_serial.get(k, 0) - st_tiled.get(k, 0) for k in ("calls", "tiles", "bytes_sent")}}
        make_shard()        # back to the default for the kernel-timing steps below
        for k in range(next_k, next_k + 3):
            step(k)
        torch.cuda.synchronize()
        next_k += 3

    # kernel-level timing for the roofline: K more steps with HIP events around every launch, recorded on the
    # stream the kernels run on (engine-side, fr_set_timing)
    hip.set_timing(True)
    hip.reset_timing()
    for k in range(next_k, next_k + K):
        step(k)
    torch.cuda.synchronize()
    bank_ms, bank_launches = hip.get_timing("bank")
    all_ms, all_launches = hip.get_timing("all")
    plan = hip.plan()
    hip.set_timing(False)
    next_k += K
    barrier()

    extras = not args.no_extras and rank == 0 and world == 1 and elapsed / K < 5e-3
    # The drop-in entry point, Renderer::fill_buffer as dispatch.rs:150 calls it: host rows in, host buffer out,
    # synchronous.  >= 100 warm calls.
    host_api = None
    if extras:
        n_host = 120
        rows = [ramp_row(next_k + i) for i in range(n_host + 10)]
        hout = np.zeros((V, T), dtype=np.float32)
        for i in range(10):
            hip.fill_buffer(V, stripe0 + (next_k + i) * T, stripe0 + (next_k + i + 1) * T, [rows[i]], out=hout)
        th = time.perf_counter()
        for i in range(10, 10 + n_host):
            hip.fill_buffer(V, stripe0 + (next_k + i) * T, stripe0 + (next_k + i + 1) * T, [rows[i]], out=hout)
        dt = time.perf_counter() - th
        host_api = {"value": n_host * T / dt / 1e6, "unit": "Msamples/s", "ms_per_step": dt / n_host * 1e3, "calls": n_host,
                    "what": "fr_fill_buffer: pageable host rows in, pageable host [V,T] buffer out, synchronous (the reference's "
                            "Renderer::fill_buffer contract, dispatch.rs:150-151); PCIe- and sync-inclusive"}
        next_k += n_host + 10
        # the same calls for a host that reuses its sample buffer and has page-locked it (fr_host_register, optional)
        hip.host_register(hout)
        rows = [ramp_row(next_k + i) for i in range(n_host + 10)]
        for i in range(10):
            hip.fill_buffer(V, stripe0 + (next_k + i) * T, stripe0 + (next_k + i + 1) * T, [rows[i]], out=hout)
        th = time.perf_counter()
        for i in range(10, 10 + n_host):
            hip.fill_buffer(V, stripe0 + (next_k + i) * T, stripe0 + (next_k + i + 1) * T, [rows[i]], out=hout)
        dt = time.perf_counter() - th
        hip.host_unregister(hout)
        host_api["registered_buffer"] = {"value": n_host * T / dt / 1e6, "ms_per_step": dt / n_host * 1e3,
                                         "what": "same calls into a buffer the host page-locked once (fr_host_register: a host that reuses its sample "
                                                 "buffer): the kernels store straight into it, no D2H copy"}
        next_k += n_host + 10

    # independent calls overlapped on two streams (an extra, never `value`)
    overlapped = None
    # (also for a voice-sharded job: a rank's share is a few-voice launch whose tail -- a handful of latency-bound waves,
    #  DESIGN.md 4.5a -- is exactly what the next call's first waves can fill; every rank runs this leg, time = max over ranks)
    stateless = not plan.get("rings") and not plan.get("stage_programs") and not plan.get("pull_rows")
    if (extras or (world > 1 and shard_mode == "voices" and not args.no_extras)) and n_streams == 1 and stateless:
        s2 = [torch.cuda.Stream(), torch.cuda.Stream()]
        o2 = [torch.empty_like(d_out), torch.empty_like(d_out)]

        def step2(k):
            row = d_time[(k % ring_steps) * T:][:T]
            hip.fill_buffer_device(o2[k % 2].data_ptr(), V, T, stripe0 + k * T, row.data_ptr(), [0, T], s2[k % 2].cuda_stream)

        for k in range(next_k, next_k + W):
            step2(k)
        torch.cuda.synchronize()
        barrier()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for k in range(next_k + W, next_k + W + K):
            step2(k)
        torch.cuda.synchronize()
        e2 = time.perf_counter() - t2
        barrier()
        e2 = max_over_ranks(e2)
        next_k += W + K
        overlapped = {"streams": 2, "value": K * T / e2 / 1e6, "unit": "Msamples/s", "ms_per_step": e2 / K * 1e3, "n_gpus": world,
                      "note": "same K steps issued round-robin on 2 HIP streams with separate output buffers; kernels of consecutive "
                              "calls overlap, so per-launch durations are not comparable with the sequential run above"}

    # short blocks ("also report T in {64, 512}"): one call through the device entry point, back to back
    short_blocks = None
    if extras:
        short_blocks = {}
        pf_rate = VALU_LANE_RATE / OPS_EXECUTED_PER_PF
        for tb in (1, 64, 512):
            base = stripe0 + (next_k + 8) * T
            for k in range(520):
                if k == 20:
                    torch.cuda.synchronize()
                    tb0 = time.perf_counter()
                row = d_time[(k * tb) % (T - tb + 1):][:tb]   # any resident f32 row of the right length will do for timing
                hip.fill_buffer_device(d_out.data_ptr(), V, tb, base + k * tb, row.data_ptr(), [0, tb], stream)
            torch.cuda.synchronize()
            us = (time.perf_counter() - tb0) / 500 * 1e6
            short_blocks[str(tb)] = {"us_per_call": us, "msamples_per_s": tb / us,
                                     "valu_frac": (float(V) * P * tb / pf_rate) / (us * 1e-6)}
            if tb == 1:   # SURVEY 8d's per-sample state-streaming accounting: 16 B per partial + 4 B per voice + 4 B, per frame
                b1 = 16.0 * V * P + 4.0 * V + 4.0
                short_blocks["1"]["hbm_frac_state_streaming_model"] = b1 / (us * 1e-6) / (HBM_PEAK_GBS * 1e9)
                short_blocks["1"]["note"] = ("one frame per call: the closed-form kernel reads 8 B per partial (no phase state); against the "
                                             "survey's 16 B-per-partial model this is the fraction of 8 TB/s; launch latency, not HBM, bounds it")
            next_k += 8 + (520 * tb) // T + 1
            # the same calls alternating between two streams (separate output buffers): calls of a plan without delay state
            # are independent, and unless the launch needs the shared chunk workspace the engine lets them overlap
            if tb == 512 and not plan.get("rings") and not plan.get("stage_programs") and not plan.get("pull_rows"):
                s2 = [torch.cuda.Stream(), torch.cuda.Stream()]
                o2 = [torch.empty_like(d_out), torch.empty_like(d_out)]
                base = stripe0 + (next_k + 8) * T
                for k in range(520):
                    if k == 20:
                        torch.cuda.synchronize()
                        tb0 = time.perf_counter()
                    row = d_time[(k * tb) % (T - tb + 1):][:tb]
                    hip.fill_buffer_device(o2[k % 2].data_ptr(), V, tb, base + k * tb, row.data_ptr(), [0, tb], s2[k % 2].cuda_stream)
                torch.cuda.synchronize()
                short_blocks[str(tb)]["two_streams_us_per_call"] = (time.perf_counter() - tb0) / 500 * 1e6
                next_k += 8 + (520 * tb) // T + 1

    # block streaming: the real-time case host to host -- one 64-frame block through fr_fill_buffer (a launch per block) and through
    # the resident launch (fr_stream_block), with the 1.3 ms between blocks a 48 kHz host leaves
    block_streaming = None
    if extras and world == 1 and args.tree == "additive":
        try:
            tb, gap = 64, 1.3e-3
            rows8 = [synth.time_ramp(k * tb, (k + 1) * tb) for k in range(8)]
            o_blk = np.zeros((V, tb), np.float32)

            def timed(call, n=250):
                ts = []
                for k in range(n):
                    t1 = time.perf_counter()
                    while time.perf_counter() - t1 < gap:
                        pass
                    t0 = time.perf_counter()
                    call(k)
                    ts.append((time.perf_counter() - t0) * 1e6)
                return float(np.median(ts[50:])), float(np.percentile(ts[50:], 99))

            base = (next_k + 64) * T
            fb = timed(lambda k: hip.fill_buffer(V, base + k * tb, base + (k + 1) * tb, [rows8[k % 8]], out=o_blk))
            hip.stream_begin(V)
            sb = timed(lambda k: hip.stream_block(base + k * tb, rows8[k % 8], out=o_blk))
            hip.stream_end()
            block_streaming = {"frames_per_block": tb, "idle_between_blocks_us": gap * 1e6,
                               "fill_buffer_us": fb[0], "fill_buffer_p99_us": fb[1], "stream_block_us": sb[0], "stream_block_p99_us": sb[1],
                               "what": "host rows in, host buffer out, synchronous, through ctypes: one launch per block vs the resident launch "
                                       "(fr_stream_begin / fr_stream_block; profiles/r02_block_streaming.txt)"}
        except Exception as e:   # an extra; never lose the line over it
            block_streaming = {"error": repr(e)}

    if rank != 0:
        if use_dist:
            dist.destroy_process_group()
        return None

    frames_total = (world if shard_mode == "time" else 1) * K * T
    value = frames_total / elapsed / 1e6
    # what THIS rank's dominant launch covers
    if shard_mode == "voices":
        pf_per_launch = float(row_hi - row_lo) * P * T
        v_launch, p_launch = row_hi - row_lo, P
    elif shard_mode == "partials":
        pf_per_launch = float(V) * (P // world) * T
        v_launch, p_launch = V, P // world
    else:
        pf_per_launch = float(V) * P * T
        v_launch, p_launch = V, P
    dom_ms, dom_n, dom_name = (bank_ms, bank_launches, "bank_kernel") if bank_launches else (all_ms, all_launches, "pull_kernel")
    avg_s = (dom_ms / max(dom_n, 1)) * 1e-3
    # algorithmic HBM bytes per launch, closed-form model of SURVEY.md 8d: parameters read once + ramp in + samples out
    bytes_per_launch = v_launch * p_launch * 8 + 4 * T + 4 * v_launch * T
    valu_rate = OPS_EXECUTED_PER_PF * pf_per_launch / avg_s if avg_s > 0 else 0.0
    roofline = {
        "bound": "valu",
        "kernel": dom_name,
        "achieved": valu_rate / 1e12,
        "peak": VALU_LANE_RATE / 1e12,
        "unit": "TFLOP/s",
        "frac": valu_rate / VALU_LANE_RATE,
        "traffic": None,
        "avg_launch_ms": avg_s * 1e3,
        "launches_timed": int(dom_n),
        "issue_frac": (ISSUE_SLOTS_PER_PF * pf_per_launch / avg_s) / VALU_LANE_RATE if avg_s > 0 else 0.0,
        "flops_per_partial_frame": {"executed_by_kernel": OPS_EXECUTED_PER_PF, "issue_slots": ISSUE_SLOTS_PER_PF,
                                    "primitive_nodes_in_graph": OPS_GRAPH_PER_PF},
        "note": "f32 VALU issue bound; peak = 256 CU x 4 SIMD x 32 lanes x 2.4 GHz lane-ops/s (the 157.3 TFLOP/s spec counts "
                "each FMA twice). achieved = executed VALU lane-ops/s (6 per partial-frame: exact algebra folds the graph's 12 "
                "primitive ops; 2 of the 6 are FMAs whose single rounding is proved equal to the graph's two). issue_frac "
                "counts v_fract_f32 as 2 slots (half rate on gfx950). The chip holds ~1.9-2.3 GHz under this load, not 2.4. "
                "MFMA not applicable: a wide reduction, no dense contraction.",
        "hbm": {"achieved": bytes_per_launch / avg_s / 1e9 if avg_s > 0 else 0.0, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": (bytes_per_launch / avg_s / 1e9) / HBM_PEAK_GBS if avg_s > 0 else 0.0,
                "algorithmic_bytes_per_launch": bytes_per_launch,
                "note": "block rendering keeps partial state in registers/SGPRs for 4800 frames: HBM is not the bound"},
    }

    # (the BASELINE.json config the line is quoted on comes first: record parsers keep the head of the string)
    same = (V, P) == (64, 4096)
    workloads = {"additive": f"BASELINE.json configs[2]{'' if same else ' shape at another size'}: {P} partials x {V} voices additive tree, 48 kHz, "
                             f"{T}-frame fill_buffer calls; harmonics and /sr as graph nodes",
                 "effects": f"BASELINE.json configs[3]{'' if (V, P) == (128, 1024) else ' shape at another size'}: harmonics + detune + ADSR + 4-tap delay chain, "
                            f"{P} partials x {V} voices, {T}-frame calls",
                 "chorus": f"diagnostic (no BASELINE config): chorus (Delay with an LFO amount) + 4-tap delay chain, {P} partials x {V} voices"}
    shardings = {"none": "single GPU",
                 "time": "time stripes: independent replicas on different frames, no collective",
                 "voices": "voices: fr_set_shard(FR_SHARD_VOICES), rank r renders its block of output rows, no collective",
                 "partials": "partials: fr_set_shard(FR_SHARD_PARTIALS), rank r renders block r of every voice's partials; recursive-halving "
                             "exchange (log2 N pairwise RCCL send/recv + the tree's own f32 add per level), bit-exact"}
    result = {
        "metric": "Msamples/sec at 4096 partials x 64 voices; achieved HBM GB/s vs roofline",
        "value": value, "unit": "Msamples/s", "n_gpus": world, "steps": K, "warmup": W,
        "ms_per_step": elapsed / K * 1e3, "higher_is_better": True,
        "scaling": "weak" if shard_mode == "time" else "strong", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": workloads[args.tree], "voices": V, "partials": P, "frames_per_call": T,
                   "sharding": shardings[shard_mode], "transport": transport, "engine_mode": args.mode,
                   "ranks": world, "launcher": launcher, "shard_world": plan.get("shard", {}).get("world"),
                   "rccl_ranks": world if transport == "rccl" else 0,
                   "rows_of_rank0": [row_lo, row_hi], "plan": plan},
        "timed": {"steps": K, "seconds": elapsed, "statistic": "one timed loop of K steps after W untimed ones",
                  "shader_clock_mhz": clock, "clock_source": "sysfs pp_dpm_sclk after the timed loop",
                  "device_warmup": {"seconds": warm_s, "calls": n_warm,
                                    "what": "the same calls on a second renderer of the tree, right before the timed loop"}},
        "partial_frames_per_s": K * T * float(V) * P * (world if shard_mode == "time" else 1) / elapsed,
        "roofline": roofline,
        "host_api": host_api,
        "short_blocks": short_blocks,
        "block_streaming": block_streaming,
        "overlapped_calls": overlapped,
        "exchange": exchange,
    }
    # BASELINE.json's other single-GPU configs as sub-records with their own roofline and parity
    if extras and not args.no_configs and args.tree == "additive":
        result["configs"] = {}
        for name in ("B", "D"):
            try:
                result["configs"][name] = other_config(name, torch, libfriendship_amd, synth, local_rank, K=max(50, min(K, 200)), W=20)
            except Exception as ex:
                result["configs"][name] = {"error": repr(ex)}
    # The HBM-bound variant of the same tree: every partial's w and amp arrive as control-rate track rows,
    # 8 bytes per partial-frame, read in place from the call's dense device matrix (fr_set_track_inputs).  The achieved
    # fraction of the HBM roofline on algorithmic bytes, at a short and a long call (tools/track_bench.py; parity:
    # tests/test_hip_parity.py::test_track_voices_against_oracle).
    if extras and not args.no_configs and args.tree == "additive" and (V, P) == (64, 4096):
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import track_bench
            tr = track_bench.run(V, P, frames=(64, 1024, 4800), steps=20, log=log)
            tr["workload"] = ("BASELINE.json configs[2] shape (64 voices x 4096 partials) with per-partial frequency / amplitude tracks as "
                              "input rows: 524289 rows x T frames per call, device-resident, 8 B per partial-frame")
            tr["roofline"] = {"bound": "hbm", "unit": "GB/s", "peak": 8000.0, "achievable": 6290.0,
                              "achieved": tr["runs"][-1]["achieved_GBps"], "frac": tr["runs"][-1]["frac_of_8TBps"],
                              "frac_of_achievable": tr["runs"][-1]["frac_of_6.29TBps"], "at_frames": tr["runs"][-1]["frames"],
                              "traffic": None}
            try:   # HBM bytes per 4800-frame launch from the committed PMC passes of tools/track_bench.py (tools/collect_profiles.sh)
                with open(PMC_SUMMARY) as f:
                    pt = json.load(f)["tracks"]
                tr["roofline"]["traffic"] = pt["derived"]["hbm_traffic_bytes"]
                tr["roofline"]["traffic_over_algorithmic"] = pt["derived"]["traffic_over_algorithmic"]
                tr["roofline"]["traffic_source"] = f"{os.path.relpath(PMC_SUMMARY, ROOT)} (rocprofv3 --pmc FETCH_SIZE x 2 [gfx950] / WRITE_SIZE, separate passes)"
            except Exception:
                pass
            result["tracks"] = tr
        except Exception as ex:
            result["tracks"] = {"error": repr(ex)}
    # HBM traffic per launch from PMC counters: rocprofv3 cannot wrap a process from inside it, so the figure is read from
    # the committed summary of the separate --pmc passes of this same command (tools/collect_profiles.sh), which records
    # the commit it was taken at.
    if (V, P, T) == (64, 4096, 4800) and world == 1:
        for path in (PMC_SUMMARY, PMC_SUMMARY.replace("r03", "r02")):
            if not os.path.exists(path):
                continue
            try:
                with open(path) as f:
                    pmc = json.load(f)
                roofline["traffic"] = pmc["derived"]["hbm_traffic_bytes"]
                roofline["traffic_source"] = (f"{os.path.relpath(path, ROOT)} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes; "
                                              f"taken at commit {pmc.get('commit', 'of round 1')})")
                break
            except Exception:
                pass

    if not args.no_cpu_baseline and world == 1:
        try:
            one, many, cpu_out = cpu_baseline(tree, V, P, args.cpu_frames, 4 * args.cpu_frames)
            result["cpu_baseline"] = one
            result["cpu_baseline_all_cores"] = many
            # parity of the bench's own paths against the CPU path on the sampled frames: the host-buffer entry point
            # (a fresh renderer, frames [0, cpu_frames)) and the device entry point
            chk = libfriendship_amd.HipRenderer(mode=args.mode, device=local_rank)
            synth.install(chk, tree)
            got = chk.fill_buffer(V, 0, args.cpu_frames, [synth.time_ramp(0, args.cpu_frames)])
            chk.close()
            chk = libfriendship_amd.HipRenderer(mode=args.mode, device=local_rank)
            synth.install(chk, tree)
            d_chk = torch.empty((V, args.cpu_frames), dtype=torch.float32, device="cuda")
            d_row = torch.from_numpy(synth.time_ramp(0, args.cpu_frames)).cuda()
            chk.fill_buffer_device(d_chk.data_ptr(), V, args.cpu_frames, 0, d_row.data_ptr(), [0, args.cpu_frames], stream)
            torch.cuda.synchronize()
            got_dev = d_chk.cpu().numpy()
            chk.close()
            result["parity"] = {"frames_checked": args.cpu_frames, "voices": V,
                                "bit_exact": bool(np.array_equal(got.view(np.uint32), cpu_out.view(np.uint32))),
                                "device_entry_bit_exact": bool(np.array_equal(got_dev.view(np.uint32), cpu_out.view(np.uint32))),
                                "against": "oracle/ref_renderer.cpp, a C++ restatement of RefRenderer (the Rust reference cannot be built here); "
                                           "pinned by the reference's own 11 tests / 14 arrays (1 x 4 samples each) and cross-checked by an "
                                           "independent numpy restatement; unpinned by any reference vector and therefore assumptions: "
                                           "f32::min on ties / NaN, NaN as u64, everything oscillator-shaped (DESIGN.md section 2)"}
        except Exception as e:   # the baseline is a reported extra; never lose the GPU line over it
            result["cpu_baseline"] = {"error": repr(e)}
    result["checksum"] = float(np.abs(last[row_lo:row_hi].astype(np.float64)).sum())
    if use_dist:
        dist.destroy_process_group()
    return json.dumps(result)


if __name__ == "__main__":
    main()
