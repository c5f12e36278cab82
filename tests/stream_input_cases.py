"""Patches for block streaming with control rows (FR_STREAM_INPUTS on top of FR_STREAM_PROGRAMS), shared by the simulator
tests of the serving rule (tests/test_stream_inputs_sim.py) and the GPU tests of the resident kernel
(tests/test_hip_stream_inputs.py).

A control row is an input slot other than 0 that a program reads at the current frame: a gain per voice, a gate, a master
volume.  All patches are at the smallest shapes the kernel serves (128 partials is its minimum).  Expectations come from the
graph:
  * `input_slots` is slot 0 (the voices' time) followed by the other slots the programs read, ascending;
  * a row that is one voice times something is ONE program of that voice (taps behind it are stored on the way);
  * a row that sums several voices of the block is one bus program and no voice programs."""
import numpy as np

import stream_bus_cases as B
import stream_cases as K
from libfriendship_amd import synth

OFF = dict(K.OPTION, FR_STREAM_BUS="1")                        # both older options, FR_STREAM_INPUTS unset: every case is refused
OPTION = dict(OFF, FR_STREAM_INPUTS="1")
STREAM_OPTIONS = dict(B.STREAM_OPTIONS, FR_STREAM_INPUTS="1")  # (with FR_STREAM_IDLE_MS=1500)
NEW_KERNEL = "bank_stream_in_kernel"
OLD_REASON = "block streaming feeds slot 0 only"


def _voices(g, V, P, seed=0x5EED0600):
    p = synth.voice_params(V, P, seed, True, wrap=24)
    return synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P))


def _times_input(g, x, slots):
    """x[v] * In(slots[v])"""
    x = np.asarray(x, dtype=np.uint32).ravel()
    y = g.nodes(synth.K_MUL, len(x))
    g.edge(x, y, 0, 0)
    g.edge(0, y, np.broadcast_to(np.asarray(slots, dtype=np.uint32), x.shape), 1)
    return y


def gain_tree(V, P, shared=False):
    """Row v = voice_v * In(1 + v) (shared: * In(1))."""
    g = synth.GraphArrays()
    y = _times_input(g, _voices(g, V, P), 1 if shared else 1 + np.arange(V))
    g.edge(y, 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def gated_taps_tree(V, P):
    """(voice * In(1)) * envelope(t), then two taps of 100 and 200 frames."""
    g = synth.GraphArrays()
    y = _times_input(g, _voices(g, V, P), 1)
    env = synth.adsr_envelope(g)
    y = g.binop(synth.K_MUL, np.broadcast_to(env, y.shape), y, V)
    y = synth.delay_chain(g, y, 2, 100.0)
    g.edge(y, 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def bus_tree(V, P):
    """(sum over v of voice_v * In(1 + v)) * In(1 + V), to one mono row."""
    g = synth.GraphArrays()
    y = _times_input(g, _voices(g, V, P), 1 + np.arange(V))
    bus = synth.sum_tree(g, np.asarray(y)[None, :])
    out = _times_input(g, bus, 1 + V)
    g.edge(out, 0, 0, 0)
    return g.finish(1)


def slots_tree(V, P, n):
    """Row v = voice_v * (In(0) * 2^-20 + In(1) + ... + In(n - 1)): one program over the slots 0 .. n - 1."""
    g = synth.GraphArrays()
    ctl = g.binop(synth.K_MUL, synth.IN(0), synth.C(np.float32(2.0 ** -20)), 1)
    for s in range(1, n):
        ctl = g.binop(synth.K_SUM2, ctl, synth.IN(s), 1)
    x = _voices(g, V, P)
    y = g.binop(synth.K_MUL, x, np.broadcast_to(ctl, x.shape), V)
    g.edge(y, 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def delayed_input_tree(V, P, d=100.0):
    """Row v = voice_v * Delay(In(1), d): a delayed read of an input row."""
    g = synth.GraphArrays()
    dl = g.binop(synth.K_DELAY, synth.IN(1), synth.C(np.float32(d)), 1)
    x = _voices(g, V, P)
    y = g.binop(synth.K_MUL, x, np.broadcast_to(dl, x.shape), V)
    g.edge(y, 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


# (name, builder, voices, output rows, input_slots, programs per voice, bus programs, workgroups)
SERVABLE = [
    ("gain_2x128", lambda: gain_tree(2, 128), 2, 2, [0, 1, 2], [1, 1], 0, 2),
    ("shared_gain_2x1024", lambda: gain_tree(2, 1024, shared=True), 2, 2, [0, 1], [1, 1], 0, 16),   # 8 chunks per voice: the finisher moves
    ("gated_taps_3x256", lambda: gated_taps_tree(3, 256), 3, 3, [0, 1], [1, 1, 1], 0, 6),
    ("bus_3x128", lambda: bus_tree(3, 128), 3, 1, [0, 1, 2, 3, 4], [0, 0, 0], 1, 3),
    ("eight_slots_2x128", lambda: slots_tree(2, 128, 8), 2, 2, list(range(8)), [1, 1], 0, 2),
]

# (name, builder, voices, output rows, fragment of the reason): refused with the option on
REFUSED = [
    ("nine_slots", lambda: slots_tree(2, 128, 9), 2, 2, "9 distinct input slots (slot 0 included); block streaming feeds at most 8"),
    ("delayed_input", lambda: delayed_input_tree(2, 128), 2, 2, "S_READ_INPUT (a delayed read of the input row)"),
]


def case(table, name):
    return K.case(table, name)


# ---- control rows ------------------------------------------------------------------------------------------------------------

HOSTILE = np.array([0.0, -0.0, 1e-42, -1e-45, np.inf, -np.inf, np.nan, 1.0, -2.5], np.float32)


def control_row(rng, T, kind):
    """One control row for a block of T frames.  kind: 0 full random, 1 short, 2 empty (continues with the slot's last value),
    3 a constant, 4 a ramp, 5 full with +-0, denormals, +-inf and NaN in it."""
    if kind == 1:
        return rng.uniform(-1.5, 1.5, size=int(rng.integers(1, T + 1))).astype(np.float32)
    if kind == 2:
        return np.zeros(0, np.float32)
    if kind == 3:
        return np.full(T, np.float32(rng.uniform(-2.0, 2.0)), np.float32)
    if kind == 4:
        return np.linspace(rng.uniform(-1, 1), rng.uniform(-1, 1), T).astype(np.float32)
    row = rng.uniform(-1.5, 1.5, size=T).astype(np.float32)
    if kind == 5:
        row[rng.integers(T, size=max(1, T // 3))] = HOSTILE[rng.integers(len(HOSTILE), size=max(1, T // 3))]
    return row


def block_inputs(rng, starts, n_in):
    """[(idx, T, rows)]: the time rows of stream_cases.block_rows (hostile values on every fifth block) and, for the slots
    1 .. n_in - 1, control rows of every kind; every slot gets a row in every block, so every block is accepted."""
    out = []
    for k, (idx, t) in enumerate(K.block_rows(rng, starts)):
        T = len(t)
        out.append((idx, T, [t] + [control_row(rng, T, int(rng.integers(6)) if k else 0) for _ in range(1, n_in)]))
    return out


def padded(row, T, last):
    """What the store makes of a row: padded with its own last value, an empty one with `last`."""
    row = np.asarray(row, np.float32)
    pad = row[-1] if len(row) else np.float32(last)
    return np.concatenate([row, np.full(T - len(row), pad, np.float32)])
