#!/usr/bin/env python3
"""Cost of feedback through Delay on the device: V additive voices of P partials, each through a comb filter
x = voice + g * Delay(x, d) -- a loop per voice, evaluated by one stage program per voice whose threads stride by d frames.
Steady 4800-frame calls (device entry point), a seek (the loops' state is rebuilt by replay from frame 0), and the same patch
without the loops (feed-forward tap) for comparison.
    python tools/feedback_bench.py [--voices 64 --partials 1024 --delays 1,32,441,2400]
                                   [--loop-tiles off|on|both --rounds 4 --stage-jit 0|force]
--loop-tiles both: FR_LOOP_TILES off and on, a renderer each per delay, measured in alternating rounds in one process (a round:
a seek to 10 s, then 50 timed steady calls); medians with min .. max of the rounds."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from libfriendship_amd import hip_lib, synth  # noqa: E402
from libfriendship_amd.capi import Renderer  # noqa: E402


def comb_tree(V, P, d, feedback=True):
    g = synth.GraphArrays()
    p = synth.voice_params(V, P, 0x5EED0300, wrap=64)
    voices = synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P))
    x = g.nodes(synth.K_SUM2, V)
    dl = g.nodes(synth.K_DELAY, V)
    m = g.binop(synth.K_MUL, dl, synth.C(np.float32(0.6)), V)
    g.edge(voices, x, 0, 0)
    g.edge(m, x, 0, 1)
    g.edge(x if feedback else voices, dl, 0, 0)      # the loop: the Delay reads x itself (feed-forward: the voice)
    g.const(dl, np.float32(d), 1)
    g.edge(x, 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def measure(r, V, T, d_out, d_t, s, torch, first_k, calls=50):
    """A seek to call `first_k`'s frames (the loops replay from 0), 5 more calls, then `calls` timed steady calls."""
    def call(k):
        r.fill_buffer_device(d_out.data_ptr(), V, T, k * T, d_t[(k % 400) * T:].data_ptr(), [0, T], s)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call(first_k)
    torch.cuda.synchronize()
    seek = time.perf_counter() - t0
    for k in range(first_k + 1, first_k + 6):
        call(k)
    torch.cuda.synchronize()
    r.set_timing(True)
    r.reset_timing()
    t0 = time.perf_counter()
    for k in range(first_k + 6, first_k + 6 + calls):
        call(k)
    torch.cuda.synchronize()
    step = (time.perf_counter() - t0) / calls
    bank_ms, nb = r.get_timing("bank")
    stage_ms, ns = r.get_timing("stage")
    r.set_timing(False)
    return {"step_us": step * 1e6, "bank_us": bank_ms / max(nb, 1) * 1e3, "stage_us": stage_ms / calls * 1e3, "launches": ns / calls, "seek_ms": seek * 1e3}


def spread(xs):
    xs = sorted(xs)
    return f"{float(np.median(xs)):8.1f} [{xs[0]:8.1f} .. {xs[-1]:8.1f}]"


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=64)
    ap.add_argument("--partials", type=int, default=1024)
    ap.add_argument("--delays", default="1,32,441,2400")
    ap.add_argument("--frames", type=int, default=4800)
    ap.add_argument("--loop-tiles", choices=("off", "on", "both"), default="off",
                    help="FR_LOOP_TILES: off, on, or both -- two renderers per delay, measured in alternating rounds in this process")
    ap.add_argument("--rounds", type=int, default=4, help="rounds per renderer: each a seek to 10 s, then 50 timed steady calls")
    ap.add_argument("--stage-jit", choices=("0", "1", "force"), default=None, help="FR_STAGE_JIT (0: the interpreter)")
    ap.add_argument("--feed-forward", type=int, default=None, help="also measure the patch without the loops (default: only with --loop-tiles off)")
    a = ap.parse_args()
    V, P, T = a.voices, a.partials, a.frames
    s = torch.cuda.current_stream().cuda_stream
    d_out = torch.empty((V, T), dtype=torch.float32, device="cuda")
    d_t = torch.from_numpy(synth.time_ramp(0, 400 * T)).cuda()
    modes = {"off": ["off"], "on": ["on"], "both": ["off", "on"]}[a.loop_tiles]
    feed_forward = a.feed_forward if a.feed_forward is not None else a.loop_tiles == "off"
    base = {} if a.stage_jit is None else {"FR_STAGE_JIT": a.stage_jit}
    for d in [int(x) for x in a.delays.split(",")]:
        tree = comb_tree(V, P, d, True)
        rs = {}
        try:
            for m in modes:
                # (off: the option left unset, the renderer every caller gets today)
                rs[m] = Renderer(hip_lib(), options={**base, **({"FR_LOOP_TILES": "1"} if m == "on" else {})})
                synth.install(rs[m], tree)
                for k in range(10):
                    rs[m].fill_buffer_device(d_out.data_ptr(), V, T, k * T, d_t[k * T:].data_ptr(), [0, T], s)
            torch.cuda.synchronize()
            res = {m: [] for m in modes}
            for rnd in range(a.rounds):
                for m in modes:      # alternating: off, on, off, on ... -- the same seek target every time (never contiguous)
                    res[m].append(measure(rs[m], V, T, d_out, d_t, s, torch, 100))
            for m in modes:
                plan = rs[m].plan()
                variants = sorted({ln["variant"] for ln in plan["stage_launches"]})
                print(f"{V} x {P}, delay {d:5d}, FEEDBACK, loop tiles {m:3s}: the loops' launches per call {spread([x['stage_us'] for x in res[m]])} us "
                      f"({res[m][0]['launches']:.0f} launches), call {spread([x['step_us'] for x in res[m]])} us, bank {spread([x['bank_us'] for x in res[m]])} us, "
                      f"call after a seek to 10 s {spread([x['seek_ms'] for x in res[m]])} ms; {a.rounds} rounds, median [min .. max]; "
                      f"fused_stride {plan['fused_stride']}, loop_tiles {plan.get('loop_tiles')}, {variants}", flush=True)
        finally:
            for r in rs.values():
                r.close()
        if feed_forward:
            with Renderer(hip_lib(), options=base) as r:
                synth.install(r, comb_tree(V, P, d, False))
                for k in range(10):
                    r.fill_buffer_device(d_out.data_ptr(), V, T, k * T, d_t[k * T:].data_ptr(), [0, T], s)
                x = measure(r, V, T, d_out, d_t, s, torch, 100)
                print(f"{V} x {P}, delay {d:5d}, feed-forward: call {x['step_us']:8.1f} us (bank {x['bank_us']:6.1f} us, stage {x['stage_us']:7.1f} us in "
                      f"{x['launches']:.0f} launches per call); call after a seek to 10 s: {x['seek_ms']:8.2f} ms", flush=True)


if __name__ == "__main__":
    main()
