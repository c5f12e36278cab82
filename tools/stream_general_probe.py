#!/usr/bin/env python3
"""Host-to-host latency of a 64-frame block of voices whose partial count is no power of two, blocks 1.3 ms apart (a 48 kHz
host's cadence).  Voices: 8 x 1000 and 24 x 100 partials (synth.additive_tree: general voices).  Each three ways:
  (a) streamed with FR_STREAM_GENERAL=1 (fr_stream_block, bank_stream_general_kernel: one workgroup per voice);
  (b) fr_fill_buffer of the same blocks on a renderer with no stream option: one gbank launch per block;
  (c) the same voice count padded to the next power of two (8 x 1024, 24 x 128), streamed on the kernel balanced voices have
      today (bank_stream_kernel: chunks over all CUs).
The expectation to confirm or refute: (a) beats (b), and (a) stays within a few microseconds (WITHIN_US) of (c).
Medians over the blocks after a warm-up, the three paths alternating in four rounds so that drift of the machine hits all of
them (only one of them renders at a time: a stream is closed while another path is timed); the spread of the four rounds'
medians is printed for each path.  The C entry points are called with the rows marshalled beforehand, so the binding's own
work is not in the numbers.  profiles/stream_general.txt keeps a run's lines.
usage: python tools/stream_general_probe.py [blocks]"""
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

import stream_general_cases as C

N = int(sys.argv[1]) if len(sys.argv) > 1 else 400
WARM, T, ROUNDS, GAP_US = 50, 64, 4, 1300
WITHIN_US = 5.0

# (voices, partials, partials padded to the next power of two)
PATCHES = [(8, 1000, 1024), (24, 100, 128)]


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


def probe(lib, V, P, P2):
    L = lib.lib
    out = np.zeros((V, T), np.float32)
    o = out.ctypes.data
    data = [synth.time_ramp(k * T, (k + 1) * T) for k in range(8)]
    offs = np.array([0, T], dtype=np.uint64)
    dp, op = [d.ctypes.data for d in data], offs.ctypes.data
    with Renderer(lib, options=C.OPTION) as s, Renderer(lib) as f, Renderer(lib) as g:
        synth.install(s, synth.additive_tree(V, P))
        synth.install(f, synth.additive_tree(V, P))
        synth.install(g, synth.additive_tree(V, P2))
        general = lambda idx, k: L.fr_stream_block(s.h, o, T, idx, dp[k], T)
        fill = lambda idx, k: L.fr_fill_buffer(f.h, o, V, T, idx, dp[k], op, 1)
        padded = lambda idx, k: L.fr_stream_block(g.h, o, T, idx, dp[k], T)
        at = {"a": 0, "b": 0, "c": 0}
        all_ = {"a": [], "b": [], "c": []}
        meds = {"a": [], "b": [], "c": []}
        plans = {}
        for _ in range(ROUNDS):
            for key, call, streamer in (("b", fill, None), ("c", padded, g), ("a", general, s)):
                if streamer:
                    streamer.stream_begin(V)
                _, at[key] = timed(call, at[key], WARM)
                x, at[key] = timed(call, at[key], N // ROUNDS)
                if streamer:
                    plans[key] = streamer.plan()
                    streamer.stream_end()
                all_[key] += x
                meds[key].append(float(np.median(x)))
        plan = plans["a"]["stream"]
        assert plan["kernel"] == C.NEW_KERNEL and plan["general_voices"] == [P] * V, plan
        med = lambda k: float(np.median(all_[k]))
        line = lambda k: f"median {med(k):6.1f} us  p99 {float(np.percentile(all_[k], 99)):6.1f} us  (rounds' medians {min(meds[k]):.1f} .. {max(meds[k]):.1f})"
        kernels_b = sorted(set(b["kernel"] for b in f.plan()["bank_launches"]))
        return [f"{V} x {P}: {N} blocks of {T} frames {GAP_US} us apart; (a) {plan['voices']} workgroups, one per voice",
                f"  (a) fr_stream_block, FR_STREAM_GENERAL=1 ({plan['kernel']}):   {line('a')}",
                f"  (b) fr_fill_buffer, no stream option ({', '.join(kernels_b)}):              {line('b')}",
                f"  (c) fr_stream_block of {V} x {P2} (bank_stream_kernel):             {line('c')}",
                f"  (a) / (b) = {med('a') / med('b'):.2f}: (a) < (b) {'CONFIRMED' if med('a') < med('b') else 'REFUTED'};  "
                f"(a) - (c) = {med('a') - med('c'):+.1f} us: within {WITHIN_US:.0f} us {'CONFIRMED' if med('a') - med('c') <= WITHIN_US else 'REFUTED'}"]


def main():
    lib = libfriendship_amd.hip_lib()
    lines = []
    for V, P, P2 in PATCHES:
        lines += probe(lib, V, P, P2)
        print("\n".join(lines[-5:]), flush=True)
    return "\n".join(lines)


if __name__ == "__main__":
    main()
