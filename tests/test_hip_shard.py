"""Partial-block sharding (FR_SHARD_PARTIALS) on the HIP kernels at real voice sizes: every rank renders its block of every
split voice into the tile-major exchange workspace, the recursive-halving exchange sums the blocks in the tree's Sum2
order.  All ranks are threads of this one process sharing the GPU (tests/shard_harness.py), the exchange over the
host-callback mailbox, time-tiled at the engine's default geometry (FR_EXCHANGE_TILES only switches tiling on for that
transport).  The per-rank block sizes are chosen so that each large-voice kernel writes the workspace:

  a   8 x 16384, world 2: blocks of 2^13, 152 (voice, tile) pairs per 1216-frame tile -> bank_short_kernel, chunks + tickets
  b   the same at world 4: blocks of 2^12, and the exchange's intermediate combine (dst_ws)
  c   64 x 4096, world 2: 2^11, 1216 pairs -> the 8-wave time-major bank_kernel
  d   4 x 65536, world 2, 65536-frame calls: 2^15 on 16384-frame tiles, 1024 pairs -> bank_kernel in 2^14 chunks + bank_combine_kernel
  e   triangle leaves 4 x 8192, world 2: hipRTC jit_bank
  f   config D's effects tree 4 x 16384 (3 taps of 2400 frames), world 2: split voices feed rings, look-back windows tiled
  mixed, world 2: split voices, a voice too small to split kept whole (rendered on the call's stream under the exchange),
      a voice two ranks need

Each case runs the call sequence of tests/shard_sequence.py (the CPU twin is test_shard_sim.py
test_default_tile_geometry_call_sequence) and is checked against the oracle by sampling, bit for bit."""
import numpy as np
import pytest

import shard_harness
import shard_sequence
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer
from shard_sequence import Call
from test_hip_parity import _triangle_tree

pytestmark = pytest.mark.gpu


def gpu_device_fill(ren, n_slots, call):
    """fr_fill_buffer_device with the row and the output in HBM, on a stream of the rank's own."""
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        row = torch.from_numpy(call.row()).cuda()
        out = torch.full((n_slots, call.n), float(shard_sequence.SENTINEL), dtype=torch.float32, device="cuda")
    s.synchronize()
    ren.fill_buffer_device(out.data_ptr(), n_slots, call.n, call.start, row.data_ptr(), [0, call.n], s.cuda_stream)
    s.synchronize()
    return out.cpu().numpy()


def _mixed_tree():
    """Rows 0, 3, 5: voices of 4096 partials (split); row 1: 32 partials (16 per rank: kept whole on rank 0); row 2 and,
    through a gain, row 4: one voice of 256 partials needed by both ranks (kept whole on both)."""
    g = synth.GraphArrays()
    p = synth.voice_params(5, 4096, 21, True)
    big = synth.sum_tree(g, synth.partial_leaves(g, p["w"][:3], p["amp"][:3]).reshape(3, 4096))
    small = synth.sum_tree(g, synth.partial_leaves(g, p["w"][3, :32], p["amp"][3, :32]).reshape(1, 32))
    shared = synth.sum_tree(g, synth.partial_leaves(g, p["w"][4, :256], p["amp"][4, :256]).reshape(1, 256))
    gain = g.binop(synth.K_MUL, shared, synth.C(np.float32(0.5)), 1)
    for src, row in ((big[0], 0), (small[0], 1), (shared[0], 2), (big[1], 3), (gain[0], 4), (big[2], 5)):
        g.edge(src, 0, 0, row)
    return g.finish(6)


# name: (tree, world, rows, rows sampled (None: all), split voices, block partials, jit, look-back, delay lags, calls)
def _case(name):
    lags14400 = (2400, 4800, 7200)
    return {
        "a": lambda: (synth.additive_tree(8, 16384, seed=11, detune=True), 2, 8, None, 8, 8192, False, None, (), None),
        "b": lambda: (synth.additive_tree(8, 16384, seed=11, detune=True), 4, 8, None, 8, 4096, False, None, (), None),
        "c": lambda: (synth.additive_tree(64, 4096), 2, 64, [0, 1, 5, 31, 32, 33, 58, 62, 63], 64, 2048, False, None, (), None),
        "d": lambda: (synth.additive_tree(4, 65536, seed=13), 2, 4, None, 4, 32768, False, None, (),
                      [Call(0, 65536), Call(65536, 65536, offset=0.5)]),
        "e": lambda: (_triangle_tree(4, 8192), 2, 4, None, 4, 4096, True, None, (), None),
        "f": lambda: (synth.effects_tree(4, 16384, taps=3, base_delay=2400.0), 2, 4, None, 4, 8192, False, 14400, lags14400, None),
        "mixed": lambda: (_mixed_tree(), 2, 6, None, 3, 2048, False, None, (), None),
    }[name.split("-")[0]]()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", ["a", "a-copied-rows", "b", "c", "d", "e", "f", "mixed"])
def test_partial_block_sharding_at_real_sizes(hip_lib, oracle_lib, name, monkeypatch):
    monkeypatch.setenv("FR_EXCHANGE_TILES", "4")          # (read when a renderer is created)
    monkeypatch.delenv("FR_EXCHANGE_MIN_TILE", raising=False)
    if name == "a-copied-rows":
        monkeypatch.setenv("FR_HOST_MAPPED", "1")         # host rows copied to the history, not deferred to the bank kernels
    tree, world, n_slots, slots, n_split, block, jit, lmax, lags, calls = _case(name)
    calls = calls or shard_sequence.standard_calls(lmax or 0)
    tiled = shard_harness.Job(hip_lib, world, "partials")
    serial = shard_harness.Job(hip_lib, world, "partials", serial_exchange=True)
    try:
        with Renderer(oracle_lib) as ref:
            for ren in tiled.ranks + serial.ranks:
                synth.install(ren, tree)
            first, _ = shard_sequence.run(tiled, ref, tree, n_slots, calls, slots=slots, lmax=lmax, lags=lags, serial=serial,
                                          device_fill=gpu_device_fill)
    finally:
        tiled.close()
        serial.close()
    for r, plan in enumerate(first):
        assert plan["shard"]["split_voices"] == n_split and plan["max_lookback"] == (lmax or 0), plan
        ws = [(b["voices"], b["partials"], b["jit"]) for b in plan["banks"] if b["to_exchange"]]
        assert ws == [(n_split, block, jit)], plan
        whole = [b for b in plan["banks"] if not b["to_exchange"]]
        assert bool(whole) == (name == "mixed"), plan
