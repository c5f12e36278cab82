#!/usr/bin/env python3
"""Host-to-host latency of a 64-frame block of patches whose feedback loops run through a Delay of a SIGNAL amount, blocks 1.3 ms
apart (a 48 kHz host's cadence).  Patches: the flanger with regeneration on an input row, no voice (tests/loop_dyn_cases.py
flanger), and synth.feedback_flanger at 16 x 1024; each at the sweep widths w = 1, 7, 16 and 63 (the proven lower bound of the
amount: base 2, 8, 17 and 64).  Each three ways:
  (a) streamed with FR_STREAM_SWEEP=1 (fr_stream_block_rows; bank_stream_sweep_fx_kernel / bank_stream_sweep_kernel);
  (b) fr_fill_buffer of the same blocks with FR_LOOP_DYN=1: a sweep launch per block (and the bank's);
  (c) the same with FR_LOOP_DYN=2: a stage launch per w frames.
Medians over the blocks after a warm-up, the three paths alternating in four rounds so that drift of the machine hits all of them
(only one of them renders at a time: the stream is closed while another path is timed); the spread of the four rounds' medians is
printed for each path.  The C entry points are called with the rows marshalled beforehand, so the binding's own work is not in the
numbers.  The hypothesis each width is marked against: the stream wins from w of about 8 up, as the constant loops did
(profiles/stream_loops.txt), and loses at w = 1, where a sweep may pay a dependent load on top of the interpreter's time per frame.
profiles/stream_sweep.txt keeps a run's lines.
usage: python tools/stream_sweep_probe.py [blocks]"""
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

import loop_dyn_cases as L
import stream_sweep_cases as C

N = int(sys.argv[1]) if len(sys.argv) > 1 else 400
WARM, T, ROUNDS, GAP_US = 50, 64, 4, 1300
BASES = {1: (2.0, 3.0), 7: (8.0, 6.0), 16: (17.0, 6.0), 63: (64.0, 6.0)}   # width -> (base, depth)


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


def probe(lib, name, install, n_rows, n_in, options, w):
    Lc = lib.lib
    out = np.zeros((n_rows, T), np.float32)
    o = out.ctypes.data
    rng = np.random.default_rng(5)
    # row 0: the time ramp (the voices' time row, the voiceless flanger's audio row is noise); row 1: the LFO's ramp
    data = []
    for k in range(8):
        ramp = synth.time_ramp(k * T, (k + 1) * T)
        rows = [ramp] if n_in == 1 else [(rng.normal(size=T) * 3).astype(np.float32), ramp]
        data.append(np.ascontiguousarray(np.concatenate(rows), dtype=np.float32))
    offs = np.arange(n_in + 1, dtype=np.uint64) * T
    dp, op = [d.ctypes.data for d in data], offs.ctypes.data
    with Renderer(lib, options=options) as s, Renderer(lib, options={"FR_LOOP_DYN": "1"}) as f, Renderer(lib, options={"FR_LOOP_DYN": "2"}) as g:
        for r in (s, f, g):
            install(r)
        stream = lambda idx, k: Lc.fr_stream_block_rows(s.h, o, T, idx, dp[k], op, n_in)
        sweep = lambda idx, k: Lc.fr_fill_buffer(f.h, o, n_rows, T, idx, dp[k], op, n_in)
        windows = lambda idx, k: Lc.fr_fill_buffer(g.h, o, n_rows, T, idx, dp[k], op, n_in)
        at = {"a": 0, "b": 0, "c": 0}
        all_ = {"a": [], "b": [], "c": []}
        meds = {"a": [], "b": [], "c": []}
        for _ in range(ROUNDS):
            for key, call in (("b", sweep), ("c", windows), ("a", stream)):
                if key == "a":
                    s.stream_begin(n_rows)
                _, at[key] = timed(call, at[key], WARM)
                x, at[key] = timed(call, at[key], N // ROUNDS)
                if key == "a":
                    plan = s.plan()["stream"]
                    s.stream_end()
                all_[key] += x
                meds[key].append(float(np.median(x)))
        assert plan["kernel"] in C.KERNELS.values() and sorted(set(x for x in plan["sweep_programs"] if x)) == [w], plan
        assert f.plan()["loop_dyn"]["form"] == "sweep" and g.plan()["loop_dyn"]["form"] == "windows"
        med = lambda k: float(np.median(all_[k]))
        line = lambda k: f"median {med(k):6.1f} us  p99 {float(np.percentile(all_[k], 99)):6.1f} us  (rounds' medians {min(meds[k]):.1f} .. {max(meds[k]):.1f})"
        best = min(med("b"), med("c"))
        wins = med("a") < best
        expected = "wins" if w >= 7 else "loses"
        verdict = "CONFIRMED" if (wins == (w >= 7)) else "REFUTED"
        return [f"{name}, w = {w}: {N} blocks of {T} frames {GAP_US} us apart; {plan['voices']} voices x {plan['chunks']} chunks, {plan['kernel']}",
                f"  (a) fr_stream_block_rows, FR_STREAM_SWEEP=1: {line('a')}",
                f"  (b) fr_fill_buffer, FR_LOOP_DYN=1 (sweeps):   {line('b')}",
                f"  (c) fr_fill_buffer, FR_LOOP_DYN=2 (windows):  {line('c')}",
                f"  (a) / min(b, c) = {med('a') / best:.2f}: the stream {'wins' if wins else 'loses'}; the hypothesis said it {expected}: {verdict}"]


def main():
    lib = libfriendship_amd.hip_lib()
    lines = []
    for w, (base, depth) in BASES.items():
        g = L.flanger(base, depth)
        lines += probe(lib, "flanger on an input row, no voice", g.install, 1, 2, C.VOICELESS, w)
        print("\n".join(lines[-5:]), flush=True)
    for w, (base, depth) in BASES.items():
        tree = synth.feedback_flanger(16, 1024, base, depth, 0.01, 0.5)
        lines += probe(lib, "feedback_flanger 16 x 1024", lambda r, tree=tree: synth.install(r, tree), 16, 1, C.VOICES, w)
        print("\n".join(lines[-5:]), flush=True)
    return "\n".join(lines)


if __name__ == "__main__":
    main()
