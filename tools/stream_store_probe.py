#!/usr/bin/env python3
"""What FR_STREAM_STORE costs and what it buys, host to host, in one process.  Nothing here is a pass criterion.
  1. Steady fr_stream_block time of 64-frame blocks, option on against off on the same build, for config C (64 voices x 1024
     partials, rows straight from the bank) and the 64 x 1024 comb of 441 frames: ROUNDS loops of N blocks each way, alternating
     (one stream at a time: the resident launch holds the device's compute units), the median of every loop, then the median of
     those with min .. max.  Off takes each plan's own kernel, on the top of the cascade and one vector store per streamed row
     more: that difference is what is measured.  If on's median lies outside off's min .. max the line says so and by how much.
  2. From an edit to the first streamed block returned (the edit, fr_stream_begin, the block), on against off, with and without
     FR_RING_KEEP: a gain constant, and the note-on of one 1024-partial voice, on 8 voices x 1024 partials each behind a tap of 100
     frames.  Off is today's seek warm-up, on the bring-up from the stored history.
  3. One relaunch: the block in which a bounded history (256 frames) slides, and the block in which an unbounded one doubles
     (2^20 frames), against the median block of the same stream.
usage: python tools/stream_store_probe.py [blocks per loop]"""
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
import stream_store_cases as S

N = int(sys.argv[1]) if len(sys.argv) > 1 else 400
WARM, T, ROUNDS = 100, 64, 5
PROGRAMS, STORE = dict(S.PROGRAMS), dict(S.STORE)


def loop(r, n_rows, idx, n, out):
    took = []
    for _ in range(n):
        row = synth.time_ramp(idx, idx + T)
        t0 = time.perf_counter()
        r.stream_block(idx, row, out=out)
        took.append((time.perf_counter() - t0) * 1e6)
        idx += T
    return took, idx


def steady(lib, name, tree, n_rows):
    out = np.zeros((n_rows, T), np.float32)
    med = {"on": [], "off": []}
    kernel = {}
    with Renderer(lib, options=STORE) as on, Renderer(lib, options=PROGRAMS) as off:
        synth.install(on, tree)
        synth.install(off, tree)
        at = {"on": 0, "off": 0}
        for _ in range(ROUNDS):
            for key, r in (("off", off), ("on", on)):
                r.stream_begin(n_rows)
                _, at[key] = loop(r, n_rows, at[key], WARM, out)
                took, at[key] = loop(r, n_rows, at[key], N, out)
                kernel[key] = r.plan()["stream"]["kernel"]
                r.stream_end()
                med[key].append(float(np.median(took)))
    a, b = np.median(med["on"]), np.median(med["off"])
    print(f"{name}: {ROUNDS} loops of {N} blocks of {T} frames each way, alternating")
    for key in ("off", "on"):
        print(f"  FR_STREAM_STORE {key:3s} ({kernel[key]}): median of the loops' medians {np.median(med[key]):6.1f} us, min .. max {min(med[key]):6.1f} .. {max(med[key]):6.1f}")
    inside = min(med["off"]) <= a <= max(med["off"])
    print(f"  on - off = {a - b:+.1f} us; on's median lies {'inside' if inside else 'OUTSIDE'} off's min .. max" +
          ("" if inside else f" (by {a - max(med['off']) if a > max(med['off']) else a - min(med['off']):+.1f} us)"))


def edit_to_block(lib, what, store, keep):
    """Microseconds from the edit to the first streamed block returned, a few times."""
    p = S.tap_patch(8, 1024, name="tap_probe")
    options = dict(STORE if store else PROGRAMS, **({"FR_RING_KEEP": "1"} if keep else {}), FR_STREAM_BANKS="1")
    n_rows, took = p.n_rows, []
    with Renderer(lib, options=options) as r:
        p.install(r)
        gains = [0.5, 0.8125]
        idx = 0
        for rep in range(4 if what == "gain" else 1):
            r.stream_begin(n_rows)
            for _ in range(40):
                r.stream_block_rows(idx, S.rows_at(p.name, 1, idx, T), n_times=T)
                idx += T
            rows = S.rows_at(p.name, 1, idx, T)
            t0 = time.perf_counter()
            if what == "gain":
                S.swap_const(p.dry[0], 0, gains[rep % 2], gains[(rep + 1) % 2])(r)
            else:
                p.edits["note_on"](r)
                n_rows = p.rows_after["note_on"]
            r.stream_begin(n_rows)
            r.stream_block_rows(idx, rows, n_times=T)
            took.append((time.perf_counter() - t0) * 1e6)
            idx += T
            continued = r.plan()["stream"].get("store", {}).get("continued")
            r.stream_end()
    return took, continued


def relaunch(lib, frames, history_frames, what, at):
    p = S.control_patch()
    control = np.random.default_rng(1).uniform(0.5, 1.5, size=frames).astype(np.float32)
    took = []
    with Renderer(lib, history_frames=history_frames, options=dict(p.options, **STORE)) as r:
        p.install(r)
        r.stream_begin(p.n_rows)
        out = np.zeros((p.n_rows, T), np.float32)
        for idx in range(0, frames, T):
            rows = [synth.time_ramp(idx, idx + T), control[idx:idx + T]]
            t0 = time.perf_counter()
            r.stream_block_rows(idx, rows, n_times=T, out=out)
            took.append((time.perf_counter() - t0) * 1e6)
        n = r.plan()["stream"]["store"]["relaunches"]
        r.stream_end()
    order = np.argsort(took)[::-1]
    print(f"{what}: {len(took)} blocks, {n} relaunches; median block {np.median(took):.1f} us; block {at}, the relaunch's, {took[at]:.0f} us; the slowest blocks after the first: " +
          ", ".join(f"block {k} {took[k]:.0f} us" for k in order[:4] if k != 0))


def main():
    lib = libfriendship_amd.hip_lib()
    steady(lib, "config C (64 x 1024, rows from the bank)", synth.additive_tree(n_voices=64, n_partials=1024), 64)
    steady(lib, "comb of 441 frames, 64 x 1024", K.comb_tree(64, 1024, 441), 64)
    for what in ("gain", "note_on"):
        for store, keep in ((False, False), (True, False), (True, True)):
            took, continued = edit_to_block(lib, what, store, keep)
            print(f"edit ({what}) to the first streamed block, FR_STREAM_STORE {'on ' if store else 'off'}{' FR_RING_KEEP' if keep else ''}: "
                  f"{', '.join(f'{t:.0f}' for t in took)} us (continued: {continued})")
    relaunch(lib, S.SLIDE_FRAMES, S.HISTORY_FRAMES, "bounded history of 256 frames, streamed past its first slide", S.SLIDE_BLOCK)
    relaunch(lib, S.DOUBLING_FRAMES, 0, "unbounded history, streamed past its first doubling", S.DOUBLING_BLOCK)


main()
