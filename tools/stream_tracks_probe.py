#!/usr/bin/env python3
"""Host-to-host latency of a synchronous 64-frame block of TRACK voices (synth.track_tree: every partial's w and amp read per
frame from its own pair of input rows), blocks 1.3 ms apart (a 48 kHz host's cadence), at 4 voices x 256 partials and 16 x 1024.
Each three ways:
  (a) streamed with FR_STREAM_TRACKS=1 (fr_stream_block_dense; bank_stream_track_kernel: the host copies the block's track rows
      into the staging, the waves read them over PCIe one partial ahead of the interpreter);
  (b) fr_fill_buffer_dense of the same blocks on the same patch without a stream option: the hipRTC-generated jit_bank kernel with
      tracks, a copy to the device and a launch per block -- the baseline, the path such a patch has had so far;
  (c) the compiled voice of the same size WITHOUT tracks (triangle partials), streamed with FR_STREAM_LEAVES=1
      (fr_stream_block_rows; bank_stream_leaf_kernel): the parent's interpreter, so (a) - (c) is what the track reads add.
Separately: the host's copy of a block's track rows (a memcpy of the same bytes between two ordinary buffers), which (a) contains.
Medians over the blocks after a warm-up, the three paths alternating in four rounds of 100 blocks so that drift of the machine hits
all of them (only one of them renders at a time); the spread of the four rounds' medians is printed for each path.  The C entry
points are called with the matrices marshalled beforehand.  Nothing is asserted about who wins: nobody had measured this.
profiles/stream_tracks.txt keeps a run's lines.
usage: python tools/stream_tracks_probe.py [blocks]"""
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

import stream_leaves_cases as L
import stream_tracks_cases as C

N = int(sys.argv[1]) if len(sys.argv) > 1 else 400
WARM, T, ROUNDS, GAP_US = 50, 64, 4, 1300
SIZES = [(4, 256), (16, 1024)]


def spin(us):
    t1 = time.perf_counter()
    while (time.perf_counter() - t1) * 1e6 < us:
        pass


def timed(call, idx, n):
    a = []
    for k in range(n):
        spin(GAP_US)
        t0 = time.perf_counter()
        st = call(idx, k % 4)
        a.append((time.perf_counter() - t0) * 1e6)
        if st != 0:
            raise RuntimeError(f"fr_status {st} at frame {idx}")
        idx += T
    return a, idx


def probe(lib, V, P):
    Lc = lib.lib
    out = np.zeros((V, T), np.float32)
    o = out.ctypes.data
    rows = 1 + 2 * V * P
    # four matrices (the time row is rewritten per block: the tracks' values do not matter to the cost)
    mats = [np.ascontiguousarray(synth.track_rows(V, P, k * T, (k + 1) * T)) for k in range(4)]
    ramps = [np.ascontiguousarray(synth.time_ramp(k * T, (k + 1) * T)) for k in range(4)]
    offs = np.arange(2, dtype=np.uint64) * T
    mp, rp, op = [m.ctypes.data for m in mats], [r.ctypes.data for r in ramps], offs.ctypes.data
    trk, tri = synth.track_tree(V, P), L.tri_tree(V, P)
    with Renderer(lib, options=C.OPTION) as s, Renderer(lib) as f, Renderer(lib, options=L.OPTION) as g:
        for r in (s, f):
            r.set_track_inputs(1)
            synth.install(r, trk)
            r.fill_buffer_dense(max(V, -(-rows // T)), 0, T, mats[0])        # every row live: n_slots * 64 >= the matrix's rows
        synth.install(g, tri)
        dense = lambda idx, k: Lc.fr_stream_block_dense(s.h, o, T, idx, mp[k], rows)
        fill = lambda idx, k: Lc.fr_fill_buffer_dense(f.h, o, V, T, idx, mp[k], rows)
        leaves = lambda idx, k: Lc.fr_stream_block_rows(g.h, o, T, idx, rp[k], op, 1)
        at = {"a": T, "b": T, "c": 0}
        all_ = {"a": [], "b": [], "c": []}
        meds = {"a": [], "b": [], "c": []}
        plan = {}
        for _ in range(ROUNDS):
            for key, call, r in (("b", fill, f), ("c", leaves, g), ("a", dense, s)):
                if key != "b":
                    r.stream_begin(V)
                _, at[key] = timed(call, at[key], WARM)
                x, at[key] = timed(call, at[key], N // ROUNDS)
                if key != "b":
                    plan[key] = r.plan()
                    r.stream_end()
                all_[key] += x
                meds[key].append(float(np.median(x)))
        sa, sc = plan["a"]["stream"], plan["c"]["stream"]
        assert sa["kernel"] == C.KERNEL and sa["tracks"]["rows"] == 2 * V * P and sc["kernel"] == L.KERNEL, (sa, sc)
        assert all(b["jit"] for b in f.plan()["banks"]), f.plan()["banks"]
        # the host's copy of a block's track rows, between two ordinary buffers
        src, dst = mats[1][1:], np.empty_like(mats[1][1:])
        copies = []
        for _ in range(200):
            t0 = time.perf_counter()
            np.copyto(dst, src)
            copies.append((time.perf_counter() - t0) * 1e6)
        wgs = sa["voices"] * sa["chunks"]
        per_wave = V * P // (wgs * 16)
        med = lambda k: float(np.median(all_[k]))
        line = lambda k: f"median {med(k):7.1f} us  p99 {float(np.percentile(all_[k], 99)):7.1f} us  (rounds' medians {min(meds[k]):.1f} .. {max(meds[k]):.1f})"
        return [f"{V} voices x {P} track partials: {N} blocks of {T} frames {GAP_US} us apart; {sa['voices']} voices x {sa['chunks']} chunks = {wgs} workgroups, "
                f"{per_wave} partials per wave, a leaf of {sa['leaf_banks'][0]['ops']} instructions and {sa['leaf_banks'][0]['track_cols']} track rows; "
                f"{sa['tracks']['rows']} staged rows = {sa['tracks']['rows'] * 256 / 2 ** 20:.2f} MiB per block",
                f"  (a) fr_stream_block_dense, FR_STREAM_TRACKS=1 ({sa['kernel']}):  {line('a')}",
                f"  (b) fr_fill_buffer_dense, the generated kernel (copy + launch per block): {line('b')}",
                f"  (c) triangle voices of the same size, FR_STREAM_LEAVES=1 ({sc['leaf_banks'][0]['ops']} instructions): {line('c')}",
                f"  the host's copy of the track rows ({src.nbytes / 2 ** 20:.2f} MiB, ordinary memory):  median {float(np.median(copies)):7.1f} us",
                f"  (a) / (b) = {med('a') / med('b'):.2f}: the streamed block {'beats' if med('a') < med('b') else 'DOES NOT beat'} fr_fill_buffer_dense at this size",
                f"  (a) - (c) = {med('a') - med('c'):.1f} us: what the track reads and the host's copy add to the parent's interpreter"]


def main():
    lib = libfriendship_amd.hip_lib()
    lines = []
    for V, P in SIZES:
        lines += probe(lib, V, P)
        print("\n".join(lines[-7:]), flush=True)
    return "\n".join(lines)


if __name__ == "__main__":
    main()
