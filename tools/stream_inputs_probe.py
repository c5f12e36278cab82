#!/usr/bin/env python3
"""Host-to-host latency of a 64-frame block with control rows through the resident launch (fr_stream_block_rows,
FR_STREAM_PROGRAMS=1 FR_STREAM_BUS=1 FR_STREAM_INPUTS=1: bank_stream_in_kernel), blocks 1.3 ms apart (a 48 kHz host's cadence),
for K = 2, 4 and 8 streamed rows (the time row and K - 1 gains) on two gain-per-voice patches: 64 x 1024, one row per voice
(4 chunks per voice = 256 workgroups), and 5 x 1024 summed to a stereo bus.  Three lines per patch and K:
  (a) fr_stream_block_rows;
  (b) the same blocks, rows included, through fr_fill_buffer of the same patch;
  (c) the same patch with the gains as constants through fr_stream_block on the existing program / bus kernels: (a) - (c) is
      what the rows themselves cost.
Medians and p99 over 1000 blocks after 200 of warm-up, the three paths alternating in four rounds so that drift of the
machine hits all of them (only one of them renders at a time: the streams are closed while another path is timed).  The C
entry points are called with rows marshalled beforehand, so the binding's own work is not in the numbers.
usage: python tools/stream_inputs_probe.py [blocks]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import libfriendship_amd
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

import stream_bus_cases as B
import stream_input_cases as I

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
WARM, T, ROUNDS, GAP_US = 200, 64, 4, 1300


def spin(us):
    t1 = time.perf_counter()
    while (time.perf_counter() - t1) * 1e6 < us:
        pass


def timed(call, idx, n):
    a = []
    for k in range(n):
        spin(GAP_US)
        t0 = time.perf_counter()
        st = call(idx, k % 8)
        a.append((time.perf_counter() - t0) * 1e6)
        if st != 0:
            raise RuntimeError(f"fr_status {st} at frame {idx}")
        idx += T
    return a, idx


def gain_patch(V, P, K, buses, constants):
    """buses == 0: row v = voice_v * gain_v; else voices b::buses * gain_v summed into bus b.  gain_v = In(1 + v % (K - 1)); where
    there are fewer voices than gains, the remaining slots are master gains of the buses, so that K rows are read in all.
    `constants`: every gain a constant instead."""
    g = synth.GraphArrays()
    p = synth.voice_params(V, P, 0x5EED0700, True, wrap=24)
    x = synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P))
    per_voice = min(V, K - 1)

    def times(h, slots, values):
        h = np.asarray(h, dtype=np.uint32).ravel()
        if constants:
            return g.binop(synth.K_MUL, synth.C(values), h, len(h))
        y = g.nodes(synth.K_MUL, len(h))
        g.edge(h, y, 0, 0)
        g.edge(0, y, np.asarray(slots, dtype=np.uint32), 1)
        return y

    y = times(x, 1 + np.arange(V) % per_voice, B.gains(V))
    if buses:
        y = np.array([synth.sum_tree(g, np.asarray(y[b::buses])[None, :])[0] for b in range(buses)], dtype=np.uint32)
        for k, slot in enumerate(range(1 + per_voice, K)):
            b = k % buses
            y[b] = times(y[b:b + 1], [slot], np.float32([0.875]))[0]
    else:
        assert per_voice == K - 1
    n_rows = buses if buses else V
    g.edge(y, 0, 0, np.arange(n_rows, dtype=np.uint32))
    return g.finish(n_rows), n_rows


def probe(name, V, P, K, buses):
    lib = libfriendship_amd.hip_lib()
    L = lib.lib
    tree, n_rows = gain_patch(V, P, K, buses, False)
    const_tree, _ = gain_patch(V, P, K, buses, True)
    out = np.zeros((n_rows, T), np.float32)
    o = out.ctypes.data
    rng = np.random.default_rng(K)
    # eight blocks' rows, marshalled once: [time, K - 1 gains] x 64 floats, CSR offsets
    data = [np.concatenate([synth.time_ramp(k * T, (k + 1) * T)] + [rng.uniform(0.25, 1.0, size=T).astype(np.float32) for _ in range(K - 1)]) for k in range(8)]
    offs = (np.arange(K + 1, dtype=np.uint64) * T)
    dp, op = [d.ctypes.data for d in data], offs.ctypes.data
    with Renderer(lib, options=I.OPTION) as s, Renderer(lib) as f, Renderer(lib, options=B.OPTION) as c:
        synth.install(s, tree)
        synth.install(f, tree)
        synth.install(c, const_tree)
        rows = lambda idx, k: L.fr_stream_block_rows(s.h, o, T, idx, dp[k], op, K)
        fill = lambda idx, k: L.fr_fill_buffer(f.h, o, n_rows, T, idx, dp[k], op, K)
        const = lambda idx, k: L.fr_stream_block(c.h, o, T, idx, dp[k], T)
        ai = bi = ci = 0
        a, b, cc = [], [], []
        for _ in range(ROUNDS):
            _, bi = timed(fill, bi, WARM)
            y, bi = timed(fill, bi, N // ROUNDS)
            s.stream_begin(n_rows)
            _, ai = timed(rows, ai, WARM)
            x, ai = timed(rows, ai, N // ROUNDS)
            plan = s.plan()["stream"]
            s.stream_end()
            c.stream_begin(n_rows)
            _, ci = timed(const, ci, WARM)
            z, ci = timed(const, ci, N // ROUNDS)
            const_kernel = c.plan()["stream"]["kernel"]
            c.stream_end()
            a += x
            b += y
            cc += z
        assert plan["kernel"] == I.NEW_KERNEL and len(plan["input_slots"]) == K, plan
        launches = len(f.plan()["bank_launches"]) + len(f.plan()["stage_launches"])
        med = lambda v: float(np.median(v))
        p99 = lambda v: float(np.percentile(v, 99))
        print(f"{name:14s} K={K}: (a) fr_stream_block_rows ({plan['kernel']}) median {med(a):6.1f} us p99 {p99(a):6.1f} | "
              f"(b) fr_fill_buffer ({launches} launches) median {med(b):6.1f} us p99 {p99(b):6.1f} | "
              f"(c) constants, fr_stream_block ({const_kernel}) median {med(cc):6.1f} us p99 {p99(cc):6.1f} | "
              f"(a)/(b) {med(a) / med(b):.2f}  (a)-(c) {med(a) - med(cc):+.2f} us", flush=True)


for K in (2, 4, 8):
    probe("64x1024 rows", 64, 1024, K, 0)
for K in (2, 4, 8):
    probe("5x1024->2 bus", 5, 1024, K, 2)
