#!/usr/bin/env python3
"""Host-to-host latency of a 64-frame block of a chorus patch -- 64 voices x 1024 partials, y = x + 0.5 * Delay(x, 400 + 300 * lfo(t)),
the Delay's amount a signal -- in 64-frame blocks 1.3 ms apart (a 48 kHz host's cadence), three ways in one process:
  (a) streamed with FR_STREAM_DYN=1 (fr_stream_block, bank_stream_dyn_kernel: one resident launch);
  (b) the same blocks through fr_fill_buffer (a bank launch and a stage launch per block);
  (c) the same patch with the amount replaced by the constant 400, streamed on the kernel it gets with FR_STREAM_PROGRAMS alone:
      what the signal read costs on top of a constant one -- its address comes from a register, so it cannot join the program's
      leading loads in flight.
Medians and p99 over 1000 blocks after 200 of warm-up, the paths alternating in four rounds so that drift of the machine hits all
(the stream is closed while fr_fill_buffer is timed: beside a resident launch its kernels may be queued behind it).
usage: python tools/stream_dyn_probe.py [blocks]"""
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

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
WARM, T, ROUNDS, GAP_US = 200, 64, 4, 1300
V, P, BASE, DEPTH = 64, 1024, 400.0, 300.0
DYN = dict(K.OPTION, FR_STREAM_DYN="1")


def constant_tree():
    """chorus_tree's voices with the amount a constant: y = x + 0.5 * Delay(x, BASE)."""
    p = synth.voice_params(V, P, 0x5EED0004, False)
    g = synth.GraphArrays()
    x = synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P))
    wet = g.binop(synth.K_DELAY, x, synth.C(np.float32(BASE)), V)
    y = g.binop(synth.K_SUM2, x, g.binop(synth.K_MUL, synth.C(np.float32(0.5)), wet, V), V)
    g.edge(y, 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


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
    chorus = synth.chorus_tree(V, P, depth=DEPTH, base=BASE)
    rows = [synth.time_ramp(k * T, (k + 1) * T) for k in range(8)]
    with Renderer(lib, options=DYN) as s, Renderer(lib) as f, Renderer(lib, options=K.OPTION) as c:
        synth.install(s, chorus)
        synth.install(f, chorus)
        synth.install(c, constant_tree())
        fill = lambda idx, row, o: f.fill_buffer(V, idx, idx + T, [row], out=o)
        took = {"a": [], "b": [], "c": []}
        at = {"a": 0, "b": 0, "c": 0}
        plans = {}
        for _ in range(ROUNDS):
            _, at["b"] = timed(fill, at["b"], WARM, rows, out)
            x, at["b"] = timed(fill, at["b"], N // ROUNDS, rows, out)
            took["b"] += x
            for key, r in (("a", s), ("c", c)):
                block = lambda idx, row, o: r.stream_block(idx, row, out=o)
                r.stream_begin(V)
                _, at[key] = timed(block, at[key], WARM, rows, out)
                x, at[key] = timed(block, at[key], N // ROUNDS, rows, out)
                plans[key] = r.plan()["stream"]
                r.stream_end()
                took[key] += x
        launches = len(f.plan()["bank_launches"]) + len(f.plan()["stage_launches"])
    line = lambda k: f"median {np.median(took[k]):6.1f} us  p99 {np.percentile(took[k], 99):6.1f} us"
    a, cc = plans["a"], plans["c"]
    print(f"chorus {V} x {P}, amount {BASE:.0f} + {DEPTH:.0f} * lfo, {T}-frame blocks {GAP_US} us apart, {N} blocks after {WARM} of warm-up in {ROUNDS} rounds")
    print(f"  (a) fr_stream_block, FR_STREAM_DYN=1 ({a['kernel']}, {a['voices'] * a['chunks']} workgroups, {a['dyn_reads']} signal reads, look-back {a['lookback']}):   {line('a')}")
    print(f"  (b) fr_fill_buffer ({launches} launches per block):   {line('b')}")
    print(f"  (c) fr_stream_block, the amount the constant {BASE:.0f} ({cc['kernel']}, {cc['voices'] * cc['chunks']} workgroups):   {line('c')}")
    print(f"  (a) / (b) of medians {np.median(took['a']) / np.median(took['b']):.2f};  (a) - (c) of medians {np.median(took['a']) - np.median(took['c']):.1f} us")


main()
