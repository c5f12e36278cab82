#!/usr/bin/env python3
"""What the track history (FR_TRACK_HISTORY) costs at config C's track shape (synth.track_tree / track_rows): per call length,
the device-resident call's time with the option off and with H = 1024 and H = 4800; the tail append's bytes (read + written)
over its time (HIP events inside the library: the "stage" timing class, which holds only track_tail_kernel for this plan)
next to a device-to-device copy of the same size in the same process; and the call after an edit that makes voice 0 feed a
delay line (its window is rebuilt through the tail).

    python tools/track_history_bench.py [--voices 64 --partials 4096 --frames 64,1024,4800 --histories 0,1024,4800 --steps 20]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from libfriendship_amd import hip_lib, synth  # noqa: E402
from libfriendship_amd.capi import Renderer, RenderError, f32_bits  # noqa: E402


def copy_gbps(torch, nbytes, reps=20):
    """Bytes read + written per second of a device-to-device copy of `nbytes` (torch's copy_ of contiguous tensors)."""
    n = max(1, nbytes // 4)
    a = torch.empty(n, dtype=torch.float32, device="cuda").uniform_()
    b = torch.empty_like(a)
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * n * 4 * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9


def run(V, P, frames, histories, steps, log=print):
    import torch
    tree = synth.track_tree(V, P)
    R = tree["n_inputs"]
    s = torch.cuda.current_stream().cuda_stream
    out = []
    for H in histories:
        with Renderer(hip_lib(), options={"FR_TRACK_HISTORY": str(H)}) as r:
            r.set_track_inputs(tree["first_track"])
            synth.install(r, tree)
            prime = -(-R // V) + 1
            d_out = torch.empty((V, prime), dtype=torch.float32, device="cuda")
            d_t = torch.arange(0, prime, dtype=torch.float32, device="cuda").reshape(1, prime)
            r.fill_buffer_device_dense(d_out.data_ptr(), V, prime, 0, d_t.data_ptr(), 1, s)
            torch.cuda.synchronize()
            idx = prime
            for T in frames:
                n_mat = int(min(8, max(1, -(-(1 << 30) // (R * T * 4)))))
                mats = []
                for k in range(n_mat):
                    gen = torch.Generator(device="cuda").manual_seed(T * 8 + k)
                    d_m = torch.empty((R, T), dtype=torch.float32, device="cuda")
                    d_m.uniform_(0.0, 0.05, generator=gen)
                    mats.append(d_m)
                d_o = torch.empty((V, T), dtype=torch.float32, device="cuda")

                def call(k):
                    nonlocal idx
                    m = mats[k % n_mat]
                    m[0] = torch.arange(idx, idx + T, dtype=torch.float32, device="cuda")
                    r.fill_buffer_device_dense(d_o.data_ptr(), V, T, idx, m.data_ptr(), R, s)
                    idx += T

                for k in range(3):
                    call(k)
                torch.cuda.synchronize()
                r.set_timing(True)
                r.reset_timing()
                t0 = time.perf_counter()
                for k in range(steps):
                    call(k)
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) / steps
                bank_ms, nb = r.get_timing("bank")
                tail_ms, nt = r.get_timing("stage")
                r.set_timing(False)
                plan = r.plan()
                rec = {"history": H, "frames": T, "call_us": round(wall * 1e6, 2), "bank_us": round(bank_ms / max(nb, 1) * 1e3, 2),
                       "tail_launches_per_call": plan["track_tail_launches"], "tail_bytes_resident": plan["track_tail_bytes"]}
                if H and nt:
                    cap = 64
                    while cap < H:
                        cap <<= 1
                    moved = 2.0 * (R - 1) * min(T, cap) * 4
                    tail_s = tail_ms / nt * 1e-3
                    rec.update({"tail_us": round(tail_s * 1e6, 2), "tail_GBps": round(moved / tail_s / 1e9, 1),
                                "copy_GBps_same_size": round(copy_gbps(torch, int(moved / 2)), 1)})
                    rec["tail_frac_of_copy"] = round(rec["tail_GBps"] / rec["copy_GBps_same_size"], 3)
                out.append(rec)
                log(json.dumps(rec))
                del mats
                torch.cuda.empty_cache()
            # an edit: voice 0 + 0.5 * Delay(voice 0, 512) -- its window now starts 512 frames before the call
            root0 = int(tree["edges"][(tree["edges"][:, 1] == 0) & (tree["edges"][:, 3] == 0)][0][0])
            h = 1 << 28
            r.on_add_node(h, "Delay")
            r.on_add_node(h + 1, "Sum2")
            r.on_add_edge(root0, h, 0, 0)
            r.on_add_edge(1, h, f32_bits(512.0), 1)
            r.on_add_edge(root0, h + 1, 0, 0)
            r.on_add_edge(h, h + 1, 0, 1)
            r.on_add_edge(h + 1, 0, 0, 0)
            T = frames[-1]
            d_m = torch.empty((R, T), dtype=torch.float32, device="cuda").uniform_(0.0, 0.05)
            d_m[0] = torch.arange(idx, idx + T, dtype=torch.float32, device="cuda")
            d_o = torch.empty((V, T), dtype=torch.float32, device="cuda")
            t0 = time.perf_counter()
            try:
                r.fill_buffer_device_dense(d_o.data_ptr(), V, T, idx, d_m.data_ptr(), R, s)
                torch.cuda.synchronize()
                rec = {"history": H, "edit_call_frames": T, "edit_call_ms": round((time.perf_counter() - t0) * 1e3, 2),
                       "bank_launches": len(r.plan()["bank_launches"])}
            except RenderError as e:
                rec = {"history": H, "edit_call_frames": T, "refused": str(e)[:160]}
            out.append(rec)
            log(json.dumps(rec))
            del d_m, d_o
            torch.cuda.empty_cache()
    return {"voices": V, "partials": P, "rows": R, "runs": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", type=int, default=64)
    ap.add_argument("--partials", type=int, default=4096)
    ap.add_argument("--frames", default="64,1024,4800")
    ap.add_argument("--histories", default="0,1024,4800")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    res = run(a.voices, a.partials, [int(x) for x in a.frames.split(",")], [int(x) for x in a.histories.split(",")], a.steps)
    if a.json:
        print(json.dumps(res))


if __name__ == "__main__":
    main()
