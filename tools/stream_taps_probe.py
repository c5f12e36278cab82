#!/usr/bin/env python3
"""Host-to-host latency of a 64-frame block of a patch that delays a COMPUTED value by fewer than 64 frames or by a signal amount
(tests/stream_taps_cases.py), two ways in one process:
  (a) streamed with FR_STREAM_TAPS=1 (fr_stream_block_rows: the plan's level form inside one resident launch, a reader behind its
      storer in the same wave; every program hop is a ring store, s_waitcnt vmcnt(0) and a load back from L2);
  (b) the same blocks through fr_fill_buffer of a renderer with no option set (a bank launch and one stage launch per level),
each with the blocks 1.3 ms apart (a 48 kHz host's cadence) and back to back.  The patches: env_fir, env_taps and bus_chorus at 64
voices x 1024 partials, and a synthetic chain of 1, 2, 3 and 4 levels behind 16 x 1024 (x_k = x_(k-1) + 0.5 * Delay(x_(k-1), k)),
whose slope over the levels is the cost of one program hop on either path.
Medians and p99 over `blocks` blocks after 200 of warm-up, the paths alternating in four rounds so that drift of the machine hits
both (the stream is closed while fr_fill_buffer is timed: beside a resident launch its kernels may be queued behind it).
The expectation was that (a) beats (b), which pays a launch per level.  One run on an MI355X (profiles/stream_taps.txt): CONFIRMED
with the blocks 1.3 ms apart (0.79 - 0.88 of the call's median); back to back it is a TIE (0.93 - 1.01: env_fir 64 x 1024 26.7 against
26.6 us) -- the stage launches of a warm queue cost 2.4 us a level, a streamed hop 2.1 us.
--fill-only: column (b) alone, for a library that does not know the option; --lib PATH: that library instead of the tree's own.
usage: python tools/stream_taps_probe.py [blocks] [--fill-only] [--lib PATH]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import libfriendship_amd
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer, RendererLib

import stream_taps_cases as C

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
FILL_ONLY = "--fill-only" in sys.argv
LIB = sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else None
if LIB in ARGS:
    ARGS.remove(LIB)
N = int(ARGS[0]) if ARGS else 1000
WARM, T, ROUNDS = 200, 64, 4
ALL = dict(C.BUS_DYN)                                            # FR_STREAM_PROGRAMS, _TAPS, _BUS, _DYN: serves every patch here

PATCHES = [("env_fir 64 x 1024", lambda: C.env_fir_tree(64, 1024), 64), ("env_taps 64 x 1024", lambda: C.env_taps_tree(64, 1024), 64),
           ("bus_chorus 64 x 1024", lambda: C.bus_chorus_tree(64, 1024), 1)] + \
          [(f"chain of {k} levels, 16 x 1024", (lambda k=k: C.chain_tree(16, 1024, k)), 16) for k in (1, 2, 3, 4)]


def spin(us):
    t1 = time.perf_counter()
    while (time.perf_counter() - t1) * 1e6 < us:
        pass


def timed(call, idx, n, rows, out, gap_us):
    a = []
    for k in range(n):
        if gap_us:
            spin(gap_us)
        t0 = time.perf_counter()
        call(idx, rows[k % 8], out)
        a.append((time.perf_counter() - t0) * 1e6)
        idx += T
    return a, idx


def probe(lib, name, build, n_rows, gap_us):
    out = np.zeros((n_rows, T), np.float32)
    tree = build()
    took = {"a": [], "b": []}
    at = {"a": 0, "b": 0}
    plan = None
    with Renderer(lib, options={} if FILL_ONLY else ALL) as s, Renderer(lib) as f:
        synth.install(s, tree)
        synth.install(f, tree)
        fill = lambda idx, r2, o: f.fill_buffer(n_rows, idx, idx + T, r2, out=o)
        block = lambda idx, r2, o: s.stream_block_rows(idx, r2, n_times=T, out=o)
        rows = [[synth.time_ramp(k * T, (k + 1) * T)] for k in range(8)]
        for _ in range(ROUNDS):
            _, at["b"] = timed(fill, at["b"], WARM, rows, out, gap_us)
            x, at["b"] = timed(fill, at["b"], N // ROUNDS, rows, out, gap_us)
            took["b"] += x
            if FILL_ONLY:
                continue
            s.stream_begin(n_rows)
            _, at["a"] = timed(block, at["a"], WARM, rows, out, gap_us)
            x, at["a"] = timed(block, at["a"], N // ROUNDS, rows, out, gap_us)
            plan = s.plan()["stream"]
            s.stream_end()
            took["a"] += x
        launches = len(f.plan()["bank_launches"]) + len(f.plan()["stage_launches"])
    line = lambda k: f"median {np.median(took[k]):6.1f} us  p99 {np.percentile(took[k], 99):6.1f} us"
    print(f"{name}: {n_rows} rows, {T}-frame blocks {'%d us apart' % gap_us if gap_us else 'back to back'}, {N} blocks after {WARM} of warm-up in {ROUNDS} rounds")
    if plan is not None:
        a, b = np.median(took["a"]), np.median(took["b"])
        print(f"  (a) fr_stream_block_rows, FR_STREAM_TAPS=1 ({plan['kernel']}, {plan['levels']} levels, {plan['short_reads']} reads below a block, "
              f"{plan['bus_programs']} bus programs):   {line('a')}")
        print(f"  (b) fr_fill_buffer ({launches} launches per block):   {line('b')}")
        print(f"  (a) / (b) of medians {a / b:.2f};  (a) < (b): {'CONFIRMED' if a < b else 'REFUTED'}")
        return a, b
    print(f"  (b) fr_fill_buffer ({launches} launches per block):   {line('b')}")
    return None, np.median(took["b"])


def main():
    lib = RendererLib(LIB) if LIB else libfriendship_amd.hip_lib()
    for gap_us in (1300, 0):
        chain = []
        for name, build, n_rows in PATCHES:
            a, b = probe(lib, name, build, n_rows, gap_us)
            if name.startswith("chain"):
                chain.append((a, b))
        hop = lambda col: np.polyfit(np.arange(1, len(chain) + 1), [c[col] for c in chain], 1)[0]
        print(f"one more level of the chain, {'%d us apart' % gap_us if gap_us else 'back to back'} (least-squares slope over 1..4 levels): "
              + ("" if FILL_ONLY else f"streamed {hop(0):+.2f} us, ") + f"fr_fill_buffer {hop(1):+.2f} us")


main()
