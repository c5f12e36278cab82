"""Patches for block streaming with mix-bus programs (FR_STREAM_BUS on top of FR_STREAM_PROGRAMS), shared by the simulator
tests of the serving rule (tests/test_stream_bus_sim.py) and the GPU tests of the resident kernel
(tests/test_hip_stream_bus.py).

A mix bus is what sits between several voices and one output row when something per-voice (a gain, an envelope, a tap) comes
before the sum: the row's program reads two or more voices of the same block.  (A plain Sum2 of bare voices is not one: the
matcher folds it into one larger voice.)  Expectations come from the graph:
  * a plain mixdown has ONE program per output row in its one-launch form, and each reads the rings of the >= 2 voices of its
    bus: B bus programs, no voice programs;
  * rows_and_bus_tree has one program per voice row (it reads its own voice only) and one for the mix row;
  * taps before or after the sum do not add programs: the one-launch form computes a row in one program and stores the
    chain's intermediate values to their rings on the way;
  * a comb behind the bus is one loop per bus: one program that reads the voices, stores the loop's ring and writes the row."""
import numpy as np

import stream_cases as K
from libfriendship_amd import synth

PROGRAMS = dict(K.OPTION)                                     # FR_STREAM_PROGRAMS alone: every case below is refused ("mix bus")
OPTION = dict(K.OPTION, FR_STREAM_BUS="1")
STREAM_OPTIONS = dict(K.STREAM_OPTIONS, FR_STREAM_BUS="1")


def gains(V):
    """One gain per voice, all different, exact in f32."""
    return (np.float32(1.0) - np.float32(0.0625) * (np.arange(V, dtype=np.float32) % np.float32(12.0))).astype(np.float32)


def _gained_voices(g, V, P, envelope, seed=0x5EED0500):
    p = synth.voice_params(V, P, seed, True, wrap=24)
    x = synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P))
    x = g.binop(synth.K_MUL, synth.C(gains(V)), x, V)
    if envelope:
        env = synth.adsr_envelope(g)
        x = g.binop(synth.K_MUL, np.broadcast_to(env, x.shape), x, V)
    return x


def _buses(g, x, B):
    """Pairwise Sum2 of voices b::B into bus b (adjacent pairs level by level, an odd one carried up)."""
    return np.array([synth.sum_tree(g, np.asarray(x[b::B])[None, :])[0] for b in range(B)], dtype=np.uint32)


def mixdown_tree(V, P, B, envelope=False, pre_taps=0, post_taps=0, base_delay=2400.0):
    """Voices x per-voice gain (x ADSR), `pre_taps` feed-forward taps per voice, voices b::B summed into bus b, `post_taps`
    taps per bus, B output rows."""
    g = synth.GraphArrays()
    x = _gained_voices(g, V, P, envelope)
    if pre_taps:
        x = synth.delay_chain(g, x, pre_taps, base_delay)
    y = _buses(g, x, B)
    if post_taps:
        y = synth.delay_chain(g, y, post_taps, base_delay)
    g.edge(y, 0, 0, np.arange(B, dtype=np.uint32))
    return g.finish(B)


def bus_comb_tree(V, P, d, B=1, fb=0.6):
    """The gained mix feeding y = bus + fb * Delay(y, d), one loop per bus."""
    g = synth.GraphArrays()
    bus = _buses(g, _gained_voices(g, V, P, False), B)
    y = g.nodes(synth.K_SUM2, B)
    dl = g.nodes(synth.K_DELAY, B)
    m = g.binop(synth.K_MUL, dl, synth.C(np.float32(fb)), B)
    g.edge(bus, y, 0, 0)
    g.edge(m, y, 0, 1)
    g.edge(y, dl, 0, 0)
    g.const(dl, np.float32(d), 1)
    g.edge(y, 0, 0, np.arange(B, dtype=np.uint32))
    return g.finish(B)


def rows_and_bus_tree(V, P):
    """Rows 0..V-1: each voice x its gain x the envelope; row V: their mix."""
    g = synth.GraphArrays()
    x = _gained_voices(g, V, P, True)
    y = _buses(g, x, 1)
    g.edge(x, 0, 0, np.arange(V, dtype=np.uint32))
    g.edge(y, 0, 0, V)
    return g.finish(V + 1)


# (name, builder, voices, output rows, programs per voice, bus programs): servable with the bus, refused ("mix bus") without
SERVABLE = [
    ("mix_2x128", lambda: mixdown_tree(2, 128, 1), 2, 1, [0, 0], 1),
    ("mix_2x128_env", lambda: mixdown_tree(2, 128, 1, envelope=True), 2, 1, [0, 0], 1),
    ("mix_3x128", lambda: mixdown_tree(3, 128, 1), 3, 1, [0] * 3, 1),
    ("mix_4x128_2", lambda: mixdown_tree(4, 128, 2), 4, 2, [0] * 4, 2),
    ("mix_4x128_2_pre", lambda: mixdown_tree(4, 128, 2, pre_taps=1, base_delay=100.0), 4, 2, [0] * 4, 2),
    ("mix_4x128_2_post", lambda: mixdown_tree(4, 128, 2, post_taps=1, base_delay=64.0), 4, 2, [0] * 4, 2),
    ("mix_8x128_2", lambda: mixdown_tree(8, 128, 2), 8, 2, [0] * 8, 2),
    ("mix_16x128_2", lambda: mixdown_tree(16, 128, 2), 16, 2, [0] * 16, 2),
    ("mix_2x1024", lambda: mixdown_tree(2, 1024, 1), 2, 1, [0, 0], 1),
    ("mix_64x128_2", lambda: mixdown_tree(64, 128, 2), 64, 2, [0] * 64, 2),
    ("mix_64x128_2_env", lambda: mixdown_tree(64, 128, 2, envelope=True), 64, 2, [0] * 64, 2),
    ("mix_64x256_2", lambda: mixdown_tree(64, 256, 2), 64, 2, [0] * 64, 2),
    ("mix_5x256_2_taps", lambda: mixdown_tree(5, 256, 2, envelope=True, pre_taps=1, post_taps=1, base_delay=300.0), 5, 2, [0] * 5, 2),
    ("rows_and_bus_3x128", lambda: rows_and_bus_tree(3, 128), 3, 4, [1] * 3, 1),
    ("bus_comb_64", lambda: bus_comb_tree(2, 128, 64), 2, 1, [0, 0], 1),
    ("bus_comb_441_2", lambda: bus_comb_tree(4, 256, 441, 2), 4, 2, [0] * 4, 2),
    ("mix_row", lambda: K.mix_tree(2, 256), 2, 2, [0, 0], 2),
]

# (name, builder, voices, output rows, fragment of the reason): refused with the bus on, too
REFUSED = [
    ("bus_comb_32", lambda: bus_comb_tree(2, 128, 32), 2, 1, "32 frames back"),
    ("chorus", lambda: synth.chorus_tree(2, 256), 2, 2, "S_READ_DYN"),
    ("small_voices", lambda: mixdown_tree(2, 64, 1), 2, 1, "at least 128 partials"),
    ("more_voices_than_cus", lambda: mixdown_tree(300, 128, 2), 300, 2, "one voice per CU"),
]


def case(table, name):
    return K.case(table, name)


def stream_against_fill_buffer(hip_lib, tree, n_rows, rows, semantics="reference", options=None):
    """The blocks through fr_stream_block of a renderer with `options` (default: both streaming options on), then -- after
    the stream is closed: nothing else renders while a launch is resident -- the same blocks through fr_fill_buffer of a
    second renderer with both options off; every sample of every block equal bit for bit.
    Returns [(idx, streamed block)] and the streaming renderer's plan."""
    from libfriendship_amd.capi import Renderer
    with Renderer(hip_lib, semantics=semantics, options=STREAM_OPTIONS if options is None else options) as s:
        synth.install(s, tree)
        s.stream_begin(n_rows)
        got = [(idx, s.stream_block(idx, row)) for idx, row in rows]
        plan = s.plan()
        s.stream_end()
    with Renderer(hip_lib, semantics=semantics) as f:
        synth.install(f, tree)
        for k, ((idx, row), (_, a)) in enumerate(zip(rows, got)):
            b = f.fill_buffer(n_rows, idx, idx + len(row), [row])
            assert K.same_bits(a, b), f"block {k} at frame {idx} (T={len(row)}): " + K.first_diff(a, b)
    return got, plan
