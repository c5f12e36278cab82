#!/usr/bin/env python3
"""Host-to-host latency of a 64-frame block of a mixed chord through the resident launch (fr_stream_block,
FR_STREAM_PROGRAMS=1 FR_STREAM_BUS=1 FR_STREAM_BANKS=1: bank_stream_banks_kernel), blocks 1.3 ms apart (a 48 kHz host's
cadence).  The chord: 8 x 1024, 16 x 512 and 32 x 256 partials, every voice with a gain and the ADSR, summed to a stereo bus.
Three lines:
  (a) the chord streamed with FR_STREAM_BANKS=1: three banks in one launch;
  (b) the same blocks through fr_fill_buffer of the same patch on the same build: three bank launches and a stage launch
      per block;
  (c) the same 56 voices as ONE bank of 1024 partials, the smaller notes padded with zero-amplitude partials -- what a host
      must do to be served without the option -- streamed on bank_stream_bus_kernel.
Medians and p99 over 1000 blocks after 200 of warm-up, the three paths alternating in four rounds so that drift of the
machine hits all of them (only one of them renders at a time: the streams are closed while another path is timed); the
spread of the four rounds' medians is printed for each path.  The C entry points are called with the rows marshalled
beforehand, so the binding's own work is not in the numbers.  profiles/stream_banks.txt keeps a run's lines.
usage: python tools/stream_banks_probe.py [blocks]"""
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

import stream_banks_cases as M
import stream_bus_cases as B

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
WARM, T, ROUNDS, GAP_US = 200, 64, 4, 1300
CHORD = [(8, 1024), (16, 512), (32, 256)]


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


def padded_tree(sizes, P, buses=2):
    """The chord of stream_banks_cases.chord_tree with every voice padded to P partials of which the ones beyond its own have
    amplitude 0: one bank."""
    g = synth.GraphArrays()
    env = synth.adsr_envelope(g)
    xs = []
    for V, Pv in sizes:
        p = synth.voice_params(V, Pv, 0x5EED0720 + Pv, True, wrap=24)
        w = np.zeros((V, P), np.float32)
        amp = np.zeros((V, P), np.float32)
        w[:, :Pv] = p["w"]
        amp[:, :Pv] = p["amp"]
        xs.append(synth.sum_tree(g, synth.partial_leaves(g, w, amp).reshape(V, P)))
    x = np.concatenate(xs)
    n = len(x)
    x = g.binop(synth.K_MUL, synth.C(B.gains(n)), x, n)
    x = g.binop(synth.K_MUL, np.broadcast_to(env, x.shape), x, n)
    y = B._buses(g, x, buses)
    g.edge(y, 0, 0, np.arange(buses, dtype=np.uint32))
    return g.finish(buses)


def main():
    lib = libfriendship_amd.hip_lib()
    L = lib.lib
    n_rows = 2
    tree = M.chord_tree(CHORD)
    pad = padded_tree(CHORD, 1024)
    out = np.zeros((n_rows, T), np.float32)
    o = out.ctypes.data
    data = [synth.time_ramp(k * T, (k + 1) * T) for k in range(8)]
    offs = np.array([0, T], dtype=np.uint64)
    dp, op = [d.ctypes.data for d in data], offs.ctypes.data
    lines = []
    with Renderer(lib, options=M.OPTION) as s, Renderer(lib) as f, Renderer(lib, options=B.OPTION) as c:
        synth.install(s, tree)
        synth.install(f, tree)
        synth.install(c, pad)
        banks = lambda idx, k: L.fr_stream_block(s.h, o, T, idx, dp[k], T)
        fill = lambda idx, k: L.fr_fill_buffer(f.h, o, n_rows, T, idx, dp[k], op, 1)
        padded = lambda idx, k: L.fr_stream_block(c.h, o, T, idx, dp[k], T)
        ai = bi = ci = 0
        a, b, cc = [], [], []
        meds = {"a": [], "b": [], "c": []}
        for _ in range(ROUNDS):
            _, bi = timed(fill, bi, WARM)
            y, bi = timed(fill, bi, N // ROUNDS)
            s.stream_begin(n_rows)
            _, ai = timed(banks, ai, WARM)
            x, ai = timed(banks, ai, N // ROUNDS)
            plan = s.plan()["stream"]
            s.stream_end()
            c.stream_begin(n_rows)
            _, ci = timed(padded, ci, WARM)
            z, ci = timed(padded, ci, N // ROUNDS)
            pad_plan = c.plan()["stream"]
            c.stream_end()
            a += x
            b += y
            cc += z
            for key, v in (("a", x), ("b", y), ("c", z)):
                meds[key].append(float(np.median(v)))
        assert plan["kernel"] == M.NEW_KERNEL and len(plan["banks"]) == 3, plan
        assert pad_plan["kernel"] == "bank_stream_bus_kernel", pad_plan
        launches = len(f.plan()["bank_launches"]) + len(f.plan()["stage_launches"])
        med = lambda v: float(np.median(v))
        p99 = lambda v: float(np.percentile(v, 99))
        spread = lambda k: f"rounds' medians {min(meds[k]):.1f} .. {max(meds[k]):.1f}"
        shape = ", ".join(f"{bk['voices']} x {bk['partials']} in {bk['chunks']} chunks" for bk in plan["banks"])
        lines.append(f"chord 8x1024 + 16x512 + 32x256 -> 2, {N} blocks of {T} frames {GAP_US} us apart, {plan['max_workgroups']} workgroups at most")
        lines.append(f"(a) fr_stream_block, FR_STREAM_BANKS=1 ({plan['kernel']}: {shape}; {plan['workgroups']} workgroups): "
                     f"median {med(a):6.1f} us  p99 {p99(a):6.1f} us  ({spread('a')})")
        lines.append(f"(b) fr_fill_buffer of the same blocks ({launches} launches per block): median {med(b):6.1f} us  p99 {p99(b):6.1f} us  ({spread('b')})")
        lines.append(f"(c) padded to one bank of 56 x 1024, fr_stream_block ({pad_plan['kernel']}: {pad_plan['voices']} voices x {pad_plan['chunks']} chunks): "
                     f"median {med(cc):6.1f} us  p99 {p99(cc):6.1f} us  ({spread('c')})")
        lines.append(f"(a)/(b) {med(a) / med(b):.2f}   (a)-(c) {med(a) - med(cc):+.2f} us")
    text = "\n".join(lines)
    print(text, flush=True)
    return text


if __name__ == "__main__":
    main()
