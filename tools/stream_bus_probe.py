#!/usr/bin/env python3
"""Host-to-host latency of a 64-frame block of a mixdown through the resident launch with mix-bus programs (fr_stream_block,
FR_STREAM_PROGRAMS=1 FR_STREAM_BUS=1: bank_stream_bus_kernel) beside the same block through fr_fill_buffer of the same patch, in
the same process: an enveloped 64 x 1024 -> 2 mixdown (4 chunks per voice = 256 workgroups; each bus program sums 32 voices
in ONE wave after the block's last voice: the serial tail this probe is there to measure) and a 5 x 1024 -> 2 one.
Blocks back to back and 1.3 ms apart (a 48 kHz host's cadence); medians and p99 over 1000 blocks after 200 of warm-up,
the two paths alternating in four rounds so that drift of the machine hits both (the stream is closed while fr_fill_buffer
is timed).  Also the per-voice form of the same voices (config D's envelope, one row per voice, no bus: bank_stream_prog_kernel),
which is what the bus tail is to be compared with.
usage: python tools/stream_bus_probe.py [blocks]"""
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

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
WARM, T, ROUNDS = 200, 64, 4


def spin(us):
    t1 = time.perf_counter()
    while (time.perf_counter() - t1) * 1e6 < us:
        pass


def timed(call, idx, n, gap_us, rows, out):
    a = []
    for k in range(n):
        if gap_us:
            spin(gap_us)
        t0 = time.perf_counter()
        call(idx, rows[k % 8], out)
        a.append((time.perf_counter() - t0) * 1e6)
        idx += T
    return a, idx


def probe(name, tree, V, options=B.OPTION):
    lib = libfriendship_amd.hip_lib()
    out = np.zeros((V, T), np.float32)
    with Renderer(lib, options=options) as s, Renderer(lib) as f:
        synth.install(s, tree)
        synth.install(f, tree)
        rows = [synth.time_ramp(k * T, (k + 1) * T) for k in range(8)]
        fill = lambda idx, row, o: f.fill_buffer(V, idx, idx + T, [row], out=o)
        block = lambda idx, row, o: s.stream_block(idx, row, out=o)
        for gap_us in (0, 1300):
            fi, si = 0, 0
            a, b = [], []
            # fr_fill_buffer only ever runs while the stream is closed: beside a resident launch its kernels may be queued
            # behind it (streams share the device's hardware queues).  Every round warms up again (the stream's first block
            # is a seek and a launch).
            for _ in range(ROUNDS):
                _, fi = timed(fill, fi, WARM, gap_us, rows, out)
                x, fi = timed(fill, fi, N // ROUNDS, gap_us, rows, out)
                s.stream_begin(V)
                _, si = timed(block, si, WARM, gap_us, rows, out)
                y, si = timed(block, si, N // ROUNDS, gap_us, rows, out)
                kernel = s.plan()["stream"]["kernel"]
                s.stream_end()
                a += x
                b += y
            launches = len(f.plan()["bank_launches"]) + len(f.plan()["stage_launches"])
            print(f"{name:22s} {gap_us:4d} us between blocks: fr_fill_buffer ({launches} launches) median {np.median(a):6.1f} us p99 {np.percentile(a, 99):6.1f} | "
                  f"fr_stream_block ({kernel}) median {np.median(b):6.1f} us p99 {np.percentile(b, 99):6.1f} | ratio of medians {np.median(b) / np.median(a):.2f}", flush=True)


probe("mixdown 64x1024->2 env", B.mixdown_tree(64, 1024, 2, envelope=True), 2)
probe("mixdown 5x1024->2 env", B.mixdown_tree(5, 1024, 2, envelope=True), 2)
probe("per voice 64x1024 env", synth.effects_tree(64, 1024, taps=0, wrap=24), 64)
