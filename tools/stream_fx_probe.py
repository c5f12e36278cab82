#!/usr/bin/env python3
"""Host-to-host latency of a 64-frame block of a patch WITHOUT A VOICE, in 64-frame blocks 1.3 ms apart (a 48 kHz host's
cadence), two ways in one process:
  (a) streamed with FR_STREAM_EFFECTS=1 (fr_stream_block_rows, bank_stream_fx_kernel: one resident launch, a workgroup of one
      wave per segment of programs);
  (b) the same blocks through fr_fill_buffer of a renderer with no option set (its stage launches per block),
for three patches made of tests/stream_fx_cases.py's echo: the feedback echo x = In(1) + g * Delay(x, 100) over 1 row and over 64
rows (row k with its own gain g_k = 0.5 - k / 256, so that no two rows are one node: 64 segments), and the comb x = In(1) + 0.5 *
Delay(x, 5) over 1 row (a loop program: the loop tiles).
Medians and p99 over 1000 blocks after 200 of warm-up, the paths alternating in four rounds so that drift of the machine hits
both (the stream is closed while fr_fill_buffer is timed: beside a resident launch its kernels may be queued behind it).
usage: python tools/stream_fx_probe.py [blocks]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import libfriendship_amd
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

import stream_fx_cases as F

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
WARM, T, ROUNDS, GAP_US = 200, 64, 4, 1300
N_IN = 2


def echoes_tree(rows, d):
    """Row k = x_k = In(1) + (0.5 - k / 256) * Delay(x_k, d): `rows` independent echoes of the one input row."""
    g = synth.GraphArrays()
    return F._rows(g, np.concatenate([F._loop_on(g, synth.IN(1), d, 0.5 - k / 256.0) for k in range(rows)]))


PATCHES = [("echo_100 x 1", lambda: echoes_tree(1, 100), 1, F.INPUTS), ("echo_100 x 64", lambda: echoes_tree(64, 100), 64, F.INPUTS),
           ("comb_5 x 1", lambda: echoes_tree(1, 5), 1, F.LOOPS)]


def spin(us):
    t1 = time.perf_counter()
    while (time.perf_counter() - t1) * 1e6 < us:
        pass


def timed(call, idx, n, rows, out):
    a = []
    for k in range(n):
        spin(GAP_US)
        t0 = time.perf_counter()
        call(idx, rows[k % 8], out)
        a.append((time.perf_counter() - t0) * 1e6)
        idx += T
    return a, idx


def probe(lib, name, build, n_rows, options):
    out = np.zeros((n_rows, T), np.float32)
    tree = build()
    rng = np.random.default_rng(100)
    rows = [[synth.time_ramp(k * T, (k + 1) * T)] + [rng.uniform(-1.0, 1.0, size=T).astype(np.float32) for _ in range(1, N_IN)] for k in range(8)]
    with Renderer(lib, options=options) as s, Renderer(lib) as f:
        synth.install(s, tree)
        synth.install(f, tree)
        fill = lambda idx, r2, o: f.fill_buffer(n_rows, idx, idx + T, r2, out=o)
        block = lambda idx, r2, o: s.stream_block_rows(idx, r2, n_times=T, out=o)
        took = {"a": [], "b": []}
        at = {"a": 0, "b": 0}
        for _ in range(ROUNDS):
            _, at["b"] = timed(fill, at["b"], WARM, rows, out)
            x, at["b"] = timed(fill, at["b"], N // ROUNDS, rows, out)
            took["b"] += x
            s.stream_begin(n_rows)
            _, at["a"] = timed(block, at["a"], WARM, rows, out)
            x, at["a"] = timed(block, at["a"], N // ROUNDS, rows, out)
            plan = s.plan()["stream"]
            s.stream_end()
            took["a"] += x
        launches = len(f.plan()["bank_launches"]) + len(f.plan()["stage_launches"])
    line = lambda k: f"median {np.median(took[k]):6.1f} us  p99 {np.percentile(took[k], 99):6.1f} us"
    a, b = np.median(took["a"]), np.median(took["b"])
    print(f"{name}: {n_rows} rows, {T}-frame blocks {GAP_US} us apart, {N} blocks after {WARM} of warm-up in {ROUNDS} rounds")
    print(f"  (a) fr_stream_block_rows, FR_STREAM_EFFECTS=1 ({plan['kernel']}, {plan['segments']} segments of one wave, loop strides "
          f"{[l for l in plan.get('loop_programs', []) if l]}):   {line('a')}")
    print(f"  (b) fr_fill_buffer ({launches} launches per block):   {line('b')}")
    print(f"  (a) / (b) of medians {a / b:.2f};  (a) < (b): {'CONFIRMED' if a < b else 'REFUTED'}")


def main():
    lib = libfriendship_amd.hip_lib()
    for name, build, n_rows, options in PATCHES:
        probe(lib, name, build, n_rows, options)


main()
