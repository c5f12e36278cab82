#!/usr/bin/env python3
"""Host-to-host latency of a 64-frame block of patches with feedback loops shorter than a block, blocks 1.3 ms apart (a 48 kHz
host's cadence).  Patches: a one-pole filter per voice at 64 x 1024; combs of d = 1, 8 and 32 frames at 16 x 1024; a one-pole on
each of the two buses of 5 x 1024 voices.  Each patch three ways:
  (a) streamed with FR_STREAM_LOOPS=1 (fr_stream_block, bank_stream_loops_kernel);
  (b) fr_fill_buffer of the same blocks, FR_LOOP_TILES off: a bank launch and a strided stage launch per block;
  (c) the same with FR_LOOP_TILES=1.
Medians over the blocks after a warm-up, the three paths alternating in four rounds so that drift of the machine hits all of
them (only one of them renders at a time: the stream is closed while another path is timed); the spread of the four rounds'
medians is printed for each path.  The C entry points are called with the rows marshalled beforehand, so the binding's own
work is not in the numbers.  profiles/stream_loops.txt keeps a run's lines.
usage: python tools/stream_loops_probe.py [blocks]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import libfriendship_amd
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

import stream_loop_cases as C

N = int(sys.argv[1]) if len(sys.argv) > 1 else 400
WARM, T, ROUNDS, GAP_US = 50, 64, 4, 1300

# (name, tree, output rows, stream options)
PATCHES = [
    ("one-pole per voice, 64 x 1024", lambda: C.comb_tree(64, 1024, 1), 64, C.OPTION),
    ("comb d = 1, 16 x 1024", lambda: C.comb_tree(16, 1024, 1), 16, C.OPTION),
    ("comb d = 8, 16 x 1024", lambda: C.comb_tree(16, 1024, 8), 16, C.OPTION),
    ("comb d = 32, 16 x 1024", lambda: C.comb_tree(16, 1024, 32), 16, C.OPTION),
    ("bus one-pole, 5 x 1024 -> 2", lambda: C.bus_one_pole_tree(5, 1024), 2, C.BUS),
]


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


def probe(lib, name, tree, n_rows, options):
    L = lib.lib
    out = np.zeros((n_rows, T), np.float32)
    o = out.ctypes.data
    data = [synth.time_ramp(k * T, (k + 1) * T) for k in range(8)]
    offs = np.array([0, T], dtype=np.uint64)
    dp, op = [d.ctypes.data for d in data], offs.ctypes.data
    with Renderer(lib, options=options) as s, Renderer(lib, options={"FR_LOOP_TILES": "0"}) as f, Renderer(lib, options={"FR_LOOP_TILES": "1"}) as g:
        for r in (s, f, g):
            synth.install(r, tree)
        stream = lambda idx, k: L.fr_stream_block(s.h, o, T, idx, dp[k], T)
        fill = lambda idx, k: L.fr_fill_buffer(f.h, o, n_rows, T, idx, dp[k], op, 1)
        tiled = lambda idx, k: L.fr_fill_buffer(g.h, o, n_rows, T, idx, dp[k], op, 1)
        at = {"a": 0, "b": 0, "c": 0}
        all_ = {"a": [], "b": [], "c": []}
        meds = {"a": [], "b": [], "c": []}
        for _ in range(ROUNDS):
            for key, call in (("b", fill), ("c", tiled), ("a", stream)):
                if key == "a":
                    s.stream_begin(n_rows)
                _, at[key] = timed(call, at[key], WARM)
                x, at[key] = timed(call, at[key], N // ROUNDS)
                if key == "a":
                    plan = s.plan()["stream"]
                    s.stream_end()
                all_[key] += x
                meds[key].append(float(np.median(x)))
        assert plan["kernel"] == C.NEW_KERNEL, plan
        tile = g.plan()["loop_tiles"]
        med = lambda k: float(np.median(all_[k]))
        line = lambda k: f"median {med(k):6.1f} us  p99 {float(np.percentile(all_[k], 99)):6.1f} us  (rounds' medians {min(meds[k]):.1f} .. {max(meds[k]):.1f})"
        strides = sorted(set(l for l in plan["loop_programs"] if l))
        best = min(med("b"), med("c"))
        return [f"{name}: {N} blocks of {T} frames {GAP_US} us apart; {plan['voices']} voices x {plan['chunks']} chunks, {plan['bus_programs']} bus programs, strides {strides}",
                f"  (a) fr_stream_block, FR_STREAM_LOOPS=1 ({plan['kernel']}): {line('a')}",
                f"  (b) fr_fill_buffer, FR_LOOP_TILES=0:                              {line('b')}",
                f"  (c) fr_fill_buffer, FR_LOOP_TILES=1 (tile of {tile['frames']} frames{'' if tile['frames'] else ': ' + tile['reason']}): {line('c')}",
                f"  (a) / min(b, c) = {med('a') / best:.2f}: (a) < min(b, c) {'CONFIRMED' if med('a') < best else 'REFUTED'}"]


def main():
    lib = libfriendship_amd.hip_lib()
    lines = []
    for name, build, n_rows, options in PATCHES:
        lines += probe(lib, name, build(), n_rows, options)
        print("\n".join(lines[-5:]), flush=True)
    return "\n".join(lines)


if __name__ == "__main__":
    main()
