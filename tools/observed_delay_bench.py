#!/usr/bin/env python3
"""Cost of Delays whose amount comes from an input (FR_DELAY_OBSERVED): V additive voices of P partials, each
y = voice + 0.5 * Delay(voice, base + depth * In(1)), in FR_MODE_AUTO with the mode on (staged: bank -> ring -> S_READ_DYN,
look-back bounded by the control values observed) and off (the pull interpreter: no bound can be proven).  Reports
steady-state Msamples/s of both through the host entry point, and the time of one call whose control row widens the
look-back (a re-plan and a rebuild of the rings' window) against a steady call.
    python tools/observed_delay_bench.py [--voices 128 --partials 1024 --frames 4800 --calls 20 --off-frames 64]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from libfriendship_amd import hip_lib, synth  # noqa: E402
from libfriendship_amd.capi import Renderer  # noqa: E402
from observed_delay_cases import delayed_voices, rows_for  # noqa: E402


def steady(r, V, T, t, calls, lo, hi):
    rows = [rows_for(t + k * T, t + (k + 1) * T, lo, hi, k) for k in range(calls)]
    t0 = time.perf_counter()
    for k in range(calls):
        r.fill_buffer(V, t + k * T, t + (k + 1) * T, rows[k])
    dt = time.perf_counter() - t0
    return dt, t + calls * T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=128)
    ap.add_argument("--partials", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=4800)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--off-frames", type=int, default=64, help="call length with the mode off (the pull interpreter is slow)")
    ap.add_argument("--off-calls", type=int, default=2)
    a = ap.parse_args()
    V, P, T = a.voices, a.partials, a.frames
    tree = delayed_voices(V, P, "affine", seed=11)
    lib = hip_lib()
    res = {"voices": V, "partials": P, "frames": T}
    with Renderer(lib, options={"FR_DELAY_OBSERVED": "1"}) as r:
        synth.install(r, tree)
        _, t = steady(r, V, T, 0, 3, 0.0, 90.0)                   # warm-up: plan, rings, compiled programs
        dt, t = steady(r, V, T, t, a.calls, 0.0, 90.0)
        res["on_msamples_per_s"] = V * T * a.calls / dt / 1e6    # voice-samples (bench.py's Msamples/s counts frames)
        res["on_mframes_per_s"] = T * a.calls / dt / 1e6
        res["on_call_ms"] = dt / a.calls * 1e3
        plan = r.plan()
        res["on_plan"] = {k: plan[k] for k in ("pull_rows", "observed_delays", "observed_lookback", "rings", "stage_jit")}
        # growth: a fresh renderer at a small look-back, then one call that widens it 32x
        with Renderer(lib, options={"FR_DELAY_OBSERVED": "1"}) as g:
            synth.install(g, tree)
            _, tg = steady(g, V, T, 0, 4, 0.0, 2.0)
            dts, tg = steady(g, V, T, tg, 1, 0.0, 2.0)
            before = g.plan()["lookback_growths"]
            dgrow, tg = steady(g, V, T, tg, 1, 0.0, 90.0)
            after = g.plan()
            res["steady_call_ms"] = dts * 1e3
            res["growth_call_ms"] = dgrow * 1e3
            res["growth"] = {"growths": after["lookback_growths"] - before, "observed_lookback": after["observed_lookback"]}
    with Renderer(lib) as r:
        synth.install(r, tree)
        Toff = a.off_frames
        steady(r, V, Toff, 0, 1, 0.0, 90.0)
        dt, _ = steady(r, V, Toff, Toff, a.off_calls, 0.0, 90.0)
        res["off_frames"] = Toff
        res["off_msamples_per_s"] = V * Toff * a.off_calls / dt / 1e6
        res["off_pull_rows"] = r.plan()["pull_rows"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
