#!/usr/bin/env python3
"""Host-to-host latency of a 64-frame block of a gated patch -- 64 voices x 1024 partials, row v = voice_v * Delay(In(1), 100), a
control row read 100 frames late -- in 64-frame blocks 1.3 ms apart (a 48 kHz host's cadence), three ways in one process:
  (a) streamed with FR_STREAM_HISTORY=1 (fr_stream_block_rows, bank_stream_hist_kernel: one resident launch that keeps a
      history of the two streamed rows);
  (b) the same blocks through fr_fill_buffer (a bank launch and a stage launch per block);
  (c) the same patch with In(1) undelayed, streamed with FR_STREAM_INPUTS=1 on bank_stream_in_kernel: what the history costs on
      top of a control row read at the current frame -- together with everything else the two kernels' compositions differ in
      (the bank table, the loop tiles' and the schedule stack's LDS).
Medians and p99 over 1000 blocks after 200 of warm-up, the paths alternating in four rounds so that drift of the machine hits all
(the stream is closed while fr_fill_buffer is timed: beside a resident launch its kernels may be queued behind it).
usage: python tools/stream_hist_probe.py [blocks]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import libfriendship_amd
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

import stream_cases as K
import stream_input_cases as I

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
WARM, T, ROUNDS, GAP_US = 200, 64, 4, 1300
V, P, DELAY = 64, 1024, 100.0
INPUTS = dict(K.OPTION, FR_STREAM_INPUTS="1")
HISTORY = dict(INPUTS, FR_STREAM_HISTORY="1")


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


def main():
    lib = libfriendship_amd.hip_lib()
    out = np.zeros((V, T), np.float32)
    delayed = I.delayed_input_tree(V, P, DELAY)
    rng = np.random.default_rng(100)
    rows = [[synth.time_ramp(k * T, (k + 1) * T), rng.uniform(0.5, 1.5, size=T).astype(np.float32)] for k in range(8)]
    with Renderer(lib, options=HISTORY) as s, Renderer(lib) as f, Renderer(lib, options=INPUTS) as c:
        synth.install(s, delayed)
        synth.install(f, delayed)
        synth.install(c, I.gain_tree(V, P, shared=True))
        fill = lambda idx, r2, o: f.fill_buffer(V, idx, idx + T, r2, out=o)
        took = {"a": [], "b": [], "c": []}
        at = {"a": 0, "b": 0, "c": 0}
        plans = {}
        for _ in range(ROUNDS):
            _, at["b"] = timed(fill, at["b"], WARM, rows, out)
            x, at["b"] = timed(fill, at["b"], N // ROUNDS, rows, out)
            took["b"] += x
            for key, r in (("a", s), ("c", c)):
                block = lambda idx, r2, o: r.stream_block_rows(idx, r2, n_times=T, out=o)
                r.stream_begin(V)
                _, at[key] = timed(block, at[key], WARM, rows, out)
                x, at[key] = timed(block, at[key], N // ROUNDS, rows, out)
                plans[key] = r.plan()["stream"]
                r.stream_end()
                took[key] += x
        launches = len(f.plan()["bank_launches"]) + len(f.plan()["stage_launches"])
    line = lambda k: f"median {np.median(took[k]):6.1f} us  p99 {np.percentile(took[k], 99):6.1f} us"
    a, cc = plans["a"], plans["c"]
    print(f"gate {V} x {P}, voice * Delay(In(1), {DELAY:.0f}), {T}-frame blocks {GAP_US} us apart, {N} blocks after {WARM} of warm-up in {ROUNDS} rounds")
    print(f"  (a) fr_stream_block_rows, FR_STREAM_HISTORY=1 ({a['kernel']}, {a['voices'] * a['chunks']} workgroups, {a['hist_reads']} delayed reads, "
          f"input look-back {a['input_lookback']}):   {line('a')}")
    print(f"  (b) fr_fill_buffer ({launches} launches per block):   {line('b')}")
    print(f"  (c) fr_stream_block_rows, In(1) undelayed ({cc['kernel']}, {cc['voices'] * cc['chunks']} workgroups):   {line('c')}")
    print(f"  (a) / (b) of medians {np.median(took['a']) / np.median(took['b']):.2f};  (a) - (c) of medians {np.median(took['a']) - np.median(took['c']):.1f} us")


main()
