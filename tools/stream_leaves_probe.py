#!/usr/bin/env python3
"""Host-to-host latency of a synchronous 64-frame block of COMPILED voices -- triangle partials (synth.triangle_leaves) --, blocks
1.3 ms apart (a 48 kHz host's cadence), at 16 voices x 1024 partials and 64 x 4096.  Each three ways:
  (a) streamed with FR_STREAM_LEAVES=1 (fr_stream_block_rows; bank_stream_leaf_kernel: the leaf interpreted per partial);
  (b) fr_fill_buffer of the same 64 frames on the same patch without a stream option: the hipRTC-generated jit_bank kernel, a launch
      per block -- the baseline, the path such a patch has had so far;
  (c) the template voice of the same size (synth.additive_tree), streamed (fr_stream_block; bank_stream_kernel): the floor, what
      the resident launch costs when the leaf is the hand-written one.
Medians over the blocks after a warm-up, the three paths alternating in four rounds so that drift of the machine hits all of them
(only one of them renders at a time: a stream is closed while another path is timed); the spread of the four rounds' medians is
printed for each path.  The C entry points are called with the rows marshalled beforehand, so the binding's own work is not in the
numbers.  From (a) - (c) the interpreter's cost is derived per partial of a wave and block (64 frames, one per lane) and per leaf
instruction.  Nothing is asserted about who wins: nobody had measured this.  profiles/stream_leaves.txt keeps a run's lines.
usage: python tools/stream_leaves_probe.py [blocks]"""
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

import stream_leaves_cases as C

N = int(sys.argv[1]) if len(sys.argv) > 1 else 400
WARM, T, ROUNDS, GAP_US = 50, 64, 4, 1300
SIZES = [(16, 1024), (64, 4096)]


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


def probe(lib, V, P):
    Lc = lib.lib
    out = np.zeros((V, T), np.float32)
    o = out.ctypes.data
    data = [np.ascontiguousarray(synth.time_ramp(k * T, (k + 1) * T)) for k in range(8)]
    offs = np.arange(2, dtype=np.uint64) * T
    dp, op = [d.ctypes.data for d in data], offs.ctypes.data
    tri, sine = C.tri_tree(V, P), synth.additive_tree(V, P)
    with Renderer(lib, options=C.OPTION) as s, Renderer(lib) as f, Renderer(lib) as g:
        synth.install(s, tri)
        synth.install(f, tri)
        synth.install(g, sine)
        leaves = lambda idx, k: Lc.fr_stream_block_rows(s.h, o, T, idx, dp[k], op, 1)
        fill = lambda idx, k: Lc.fr_fill_buffer(f.h, o, V, T, idx, dp[k], op, 1)
        floor = lambda idx, k: Lc.fr_stream_block(g.h, o, T, idx, dp[k], T)
        at = {"a": 0, "b": 0, "c": 0}
        all_ = {"a": [], "b": [], "c": []}
        meds = {"a": [], "b": [], "c": []}
        plan = {}
        for _ in range(ROUNDS):
            for key, call, r in (("b", fill, f), ("c", floor, g), ("a", leaves, s)):
                if key != "b":
                    r.stream_begin(V)
                _, at[key] = timed(call, at[key], WARM)
                x, at[key] = timed(call, at[key], N // ROUNDS)
                if key != "b":
                    plan[key] = r.plan()
                    r.stream_end()
                all_[key] += x
                meds[key].append(float(np.median(x)))
        sa = plan["a"]["stream"]
        assert sa["kernel"] == C.KERNEL and sa["leaf_banks"] and all(b["jit"] for b in f.plan()["banks"]), (sa, f.plan()["banks"])
        ops = sa["leaf_banks"][0]["ops"]
        wgs = sa["voices"] * sa["chunks"]
        per_wave = V * P // (wgs * 16)
        med = lambda k: float(np.median(all_[k]))
        line = lambda k: f"median {med(k):7.1f} us  p99 {float(np.percentile(all_[k], 99)):7.1f} us  (rounds' medians {min(meds[k]):.1f} .. {max(meds[k]):.1f})"
        extra = med("a") - med("c")
        return [f"{V} voices x {P} triangle partials: {N} blocks of {T} frames {GAP_US} us apart; {sa['voices']} voices x {sa['chunks']} chunks = {wgs} workgroups, "
                f"{per_wave} partials per wave, a leaf of {ops} instructions over {sa['leaf_banks'][0]['regs']} registers",
                f"  (a) fr_stream_block_rows, FR_STREAM_LEAVES=1 ({sa['kernel']}): {line('a')}",
                f"  (b) fr_fill_buffer, the compiled kernel (a launch per block):          {line('b')}",
                f"  (c) the template voice of the same size, streamed (the floor):         {line('c')}",
                f"  (a) / (b) = {med('a') / med('b'):.2f}: the streamed block {'beats' if med('a') < med('b') else 'DOES NOT beat'} fr_fill_buffer at this size",
                f"  (a) - (c) = {extra:.1f} us for {per_wave} partials per wave: {1e3 * extra / per_wave:.1f} ns per partial and block of a wave (64 frames), "
                f"{1e3 * extra / per_wave / ops:.2f} ns per leaf instruction"]


def main():
    lib = libfriendship_amd.hip_lib()
    lines = []
    for V, P in SIZES:
        lines += probe(lib, V, P)
        print("\n".join(lines[-6:]), flush=True)
    return "\n".join(lines)


if __name__ == "__main__":
    main()
