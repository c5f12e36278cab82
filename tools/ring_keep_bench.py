#!/usr/bin/env python3
"""What FR_RING_KEEP saves: wall time of the call that follows (a) a gain edit of one voice, (b) a note-on of
one voice, (c) a re-plan with an unchanged graph (what a finished run-time compile causes), with the option off and on in the
same process, at two session positions (10 s and 100 s of audio at 48 kHz).  Two patches: config D's shape (V voices x P
partials, envelope, four taps to 24 000 frames) and the comb patch of tools/feedback_bench.py (x = voice + 0.6 Delay(x, d)) with
a gain behind every loop.  Every figure is the median of the edits with their min .. max; the launches of the timed call are
printed with it (the work is what the tests check; the times are only measured here).
    python tools/ring_keep_bench.py [--patch effects|comb --voices V --partials P --delay d --positions 10,100 --edits 20]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from libfriendship_amd import hip_lib, synth  # noqa: E402
from libfriendship_amd.capi import Renderer, f32_bits  # noqa: E402
from libfriendship_amd.synth import C, K_DELAY, K_MUL, K_SUM2  # noqa: E402

SR = 48000


def chain(g, x, taps, base):
    for j in range(taps):
        dl = g.binop(K_DELAY, x, C(np.float32(base * (j + 1))), len(x))
        x = g.binop(K_SUM2, x, g.binop(K_MUL, C(np.float32(0.5 ** (j + 1))), dl, len(x)), len(x))
    return x


def effects_patch(V, P):
    """Config D's shape with a gain per voice between the envelope and the taps (the knob the edit turns)."""
    g = synth.GraphArrays()
    p = synth.voice_params(V, P, 0x5EED0003, True, wrap=64)
    x = synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P))
    env = synth.adsr_envelope(g)
    x = g.binop(K_MUL, np.broadcast_to(env, x.shape), x, V)
    knob = g.binop(K_MUL, C(np.full(V, 0.7, np.float32)), x, V)
    g.edge(chain(g, knob, 4, 2400.0), 0, 0, np.arange(V, dtype=np.uint32))
    return g, g.finish(V), knob


def comb_patch(V, P, d):
    g = synth.GraphArrays()
    p = synth.voice_params(V, P, 0x5EED0300, wrap=64)
    voices = synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P))
    x = g.nodes(K_SUM2, V)
    dl = g.binop(K_DELAY, x, C(np.float32(d)), V)
    g.edge(voices, x, 0, 0)
    g.edge(g.binop(K_MUL, dl, C(np.float32(0.6)), V), x, 0, 1)
    knob = g.binop(K_MUL, C(np.full(V, 0.7, np.float32)), x, V)     # a gain behind each loop, outside it
    g.edge(knob, 0, 0, np.arange(V, dtype=np.uint32))
    return g, g.finish(V), knob


def new_voice(g, P, row, kind, d, seed):
    """One more voice of the patch's kind on output row `row` (handles continue after g's)."""
    h = synth.GraphArrays()
    h.next = g.next
    h.handles, h.kinds = [], []
    p = synth.voice_params(1, P, seed)
    x = synth.sum_tree(h, synth.partial_leaves(h, p["w"], p["amp"]).reshape(1, P))
    if kind == "effects":
        x = chain(h, h.binop(K_MUL, C(np.float32(0.7)), x, 1), 4, 2400.0)
    else:
        s = h.nodes(K_SUM2, 1)
        dl = h.binop(K_DELAY, s, C(np.float32(d)), 1)
        h.edge(x, s, 0, 0)
        h.edge(h.binop(K_MUL, dl, C(np.float32(0.6)), 1), s, 0, 1)
        x = h.binop(K_MUL, C(np.float32(0.7)), s, 1)
    h.edge(x, 0, 0, row)
    g.next = h.next
    return {"handles": np.concatenate(h.handles), "kinds": np.concatenate(h.kinds),
            "edges": np.ascontiguousarray(np.concatenate(h.edges, axis=0), dtype=np.uint32)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--patch", default="comb", choices=["effects", "comb"])
    ap.add_argument("--voices", type=int, default=None)
    ap.add_argument("--partials", type=int, default=None)
    ap.add_argument("--delay", type=int, default=441)
    ap.add_argument("--frames", type=int, default=4800)
    ap.add_argument("--positions", default="10,100", help="seconds of audio rendered before the edits")
    ap.add_argument("--edits", type=int, default=20)
    ap.add_argument("--note-ons", type=int, default=3)
    a = ap.parse_args()
    V = a.voices or (1024 if a.patch == "effects" else 64)
    P = a.partials or (128 if a.patch == "effects" else 1024)
    T = a.frames
    s = torch.cuda.current_stream().cuda_stream
    positions = [int(float(x) * SR) // T * T for x in a.positions.split(",")]
    last = max(positions) + (3 * a.edits + 2 * a.note_ons + 60) * T
    d_t = torch.from_numpy(synth.time_ramp(0, last)).cuda()
    d_out = torch.empty((V + a.note_ons, T), dtype=torch.float32, device="cuda")
    name = f"{a.patch} {V} x {P}" + (f", d = {a.delay}" if a.patch == "comb" else ", four taps to 24000 frames")
    for pos in positions:
        for opt in ("0", "1"):
            g, tree, knob = effects_patch(V, P) if a.patch == "effects" else comb_patch(V, P, a.delay)
            with Renderer(hip_lib(), options={"FR_RING_KEEP": opt}) as r:
                synth.install(r, tree)
                idx, n = 0, V

                def call():
                    nonlocal idx
                    t0 = time.perf_counter()
                    r.fill_buffer_device(d_out.data_ptr(), n, T, idx, d_t[idx:].data_ptr(), [0, T], s)
                    torch.cuda.synchronize()
                    idx += T
                    return (time.perf_counter() - t0) * 1e3

                while idx < pos:
                    r.fill_buffer_device(d_out.data_ptr(), n, T, idx, d_t[idx:].data_ptr(), [0, T], s)
                    idx += T
                torch.cuda.synchronize()
                steady = [call() for _ in range(20)]

                def work(p):
                    forms = {}
                    for b in p["bank_launches"]:
                        k = "bank/" + b.get("form", "call")
                        forms[k] = forms.get(k, 0) + b["voices"] * b["frames"]
                    for st in p["stage_launches"]:
                        k = "stage/" + st["form"]
                        forms[k] = forms.get(k, 0) + st["programs"] * st["frames"]
                    return ", ".join(f"{k} {v}" for k, v in sorted(forms.items()))

                def report(what, ms, p):
                    print(f"{name} | after {pos / SR:5.1f} s | FR_RING_KEEP={opt} | {what:34s} | median {np.median(ms):9.3f} ms  min {min(ms):9.3f}  max {max(ms):9.3f}"
                          f"  ({len(ms)} edits) | voice-frames / program-frames launched: {work(p)}", flush=True)

                report("steady call", steady, r.plan())
                gain, ms = np.float32(0.7), []
                for i in range(a.edits):                 # (a) the gain of voice 5: outside every loop
                    new = np.float32(0.3 + 0.01 * i)
                    r.on_del_edge(synth.CONST_HANDLE, int(knob[5]), f32_bits(gain), 0)
                    r.on_add_edge(synth.CONST_HANDLE, int(knob[5]), f32_bits(new), 0)
                    gain = new
                    ms.append(call())
                    p = r.plan()
                    call()
                report("call after a gain edit of one voice", ms, p)
                ms = []
                for i in range(max(a.edits // 2, 1)):    # (c) the same constant written again: a new plan of the same graph
                    r.on_del_edge(synth.CONST_HANDLE, int(knob[5]), f32_bits(gain), 0)
                    r.on_add_edge(synth.CONST_HANDLE, int(knob[5]), f32_bits(gain), 0)
                    ms.append(call())
                    p = r.plan()
                    call()
                report("call after an unchanged re-plan", ms, p)
                ms = []
                for i in range(a.note_ons):              # (b) one more voice on one more row
                    synth.install(r, new_voice(g, P, n, a.patch, a.delay, 0x5EED0400 + i))
                    n += 1
                    ms.append(call())
                    p = r.plan()
                    call()
                report("call after a note-on of one voice", ms, p)


if __name__ == "__main__":
    main()
