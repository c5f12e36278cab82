#!/usr/bin/env python3
"""Cost of feedback through a Delay of a SIGNAL amount (FR_LOOP_DYN): tools/feedback_bench.py's patch with the
flanger loop -- V additive voices of P partials, each through x = voice + g * Delay(x, (W + 1) + 6 * lfo(t)), whose proven
bound is W frames -- in steady 4800-frame calls.  FR_LOOP_DYN=1 (stage_sweep_kernel: one launch, a workgroup per loop, a barrier
per min(W, 256) frames) against FR_LOOP_DYN=2 (stage_kernel, one launch per W frames), a renderer each, measured in alternating
rounds in one process; medians with min .. max of the rounds.  A third column: the constant-delay comb of d = W on the
interpreter's strided launch (4.7's table), the loop the sweep form would be if the amount were a constant.
    python tools/loop_dyn_probe.py [--voices 64 --partials 1024 --bounds 1,7,16,64,256,2400 --rounds 3 --calls 20]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from libfriendship_amd import hip_lib, synth  # noqa: E402
from libfriendship_amd.capi import Renderer  # noqa: E402
from feedback_bench import comb_tree, spread  # noqa: E402


def measure(r, V, T, d_out, d_t, s, torch, first_k, calls):
    """`calls` timed steady calls from call `first_k` on (the renderer's rings are current: the caller keeps the calls contiguous)."""
    def call(k):
        r.fill_buffer_device(d_out.data_ptr(), V, T, k * T, d_t[(k % 400) * T:].data_ptr(), [0, T], s)

    torch.cuda.synchronize()
    r.set_timing(True)
    r.reset_timing()
    t0 = time.perf_counter()
    for k in range(first_k, first_k + calls):
        call(k)
    torch.cuda.synchronize()
    step = (time.perf_counter() - t0) / calls
    stage_ms, ns = r.get_timing("stage")
    r.set_timing(False)
    return {"step_us": step * 1e6, "stage_us": stage_ms / calls * 1e3, "launches": ns / calls}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=64)
    ap.add_argument("--partials", type=int, default=1024)
    ap.add_argument("--bounds", default="1,7,16,64,256,2400", help="the proven bounds W to measure")
    ap.add_argument("--frames", type=int, default=4800)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20, help="timed steady calls per round and renderer")
    a = ap.parse_args()
    V, P, T = a.voices, a.partials, a.frames
    s = torch.cuda.current_stream().cuda_stream
    d_out = torch.empty((V, T), dtype=torch.float32, device="cuda")
    d_t = torch.from_numpy(synth.time_ramp(0, 400 * T)).cuda()
    forms = {"sweep": {"FR_LOOP_DYN": "1"}, "windows": {"FR_LOOP_DYN": "2"}, "comb": {"FR_STAGE_JIT": "0"}}
    for W in [int(x) for x in a.bounds.split(",")]:
        trees = {"sweep": synth.feedback_flanger(V, P, float(W + 1), 6.0, 1e-4, 0.5), "comb": comb_tree(V, P, W, True)}
        trees["windows"] = trees["sweep"]
        rs = {}
        try:
            nxt = {}
            for m, opts in forms.items():
                rs[m] = Renderer(hip_lib(), options=opts)
                synth.install(rs[m], trees[m])
                for k in range(3):      # from frame 0, contiguous: no replay is ever timed
                    rs[m].fill_buffer_device(d_out.data_ptr(), V, T, k * T, d_t[k * T:].data_ptr(), [0, T], s)
                nxt[m] = 3
            torch.cuda.synchronize()
            res = {m: [] for m in forms}
            for rnd in range(a.rounds):
                for m in forms:         # alternating: sweep, windows, comb, sweep ...
                    res[m].append(measure(rs[m], V, T, d_out, d_t, s, torch, nxt[m], a.calls))
                    nxt[m] += a.calls
            for m in forms:
                plan = rs[m].plan()
                variants = sorted({ln["variant"] for ln in plan["stage_launches"]})
                what = f"loop_dyn {plan['loop_dyn']['form']:7s} W {plan['loop_dyn']['sweep']:5d}" if m != "comb" else f"constant comb d = {W:5d}     "
                print(f"{V} x {P}, W {W:5d}, {what}: the loops' launches per call {spread([x['stage_us'] for x in res[m]])} us "
                      f"({res[m][0]['launches']:.0f} launches), call {spread([x['step_us'] for x in res[m]])} us; {a.rounds} rounds of {a.calls} calls, "
                      f"median [min .. max]; {variants}", flush=True)
        finally:
            for r in rs.values():
                r.close()


if __name__ == "__main__":
    main()
