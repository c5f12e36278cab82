"""Patches for block streaming of Delays by a signal amount (FR_STREAM_DYN on top of FR_STREAM_PROGRAMS), shared by the simulator
tests of the serving rule (tests/test_stream_dyn_sim.py) and the GPU tests of the resident kernel (tests/test_hip_stream_dyn.py).
Graph recipes and plain data: importable without a GPU.

A chorus, a flanger, a vibrato, a delay time on a knob: Delay(voice, amount(t)) with the amount a SIGNAL.  The planner proves a
bound for the amount, keeps the voice in a ring with that look-back and emits S_READ_DYN (a Delay of a constant: S_STEP_DYN).
Voices have 128 partials, the smallest the chunked kernels serve, unless a case is about another size.  Expectations come from
the graph:
  * a row that is one voice plus a signal delay of the SAME voice is one program of that voice with one S_READ_DYN, whatever the
    bound (400..700 frames or 0..5): the offset may always be below a block;
  * a row that delays ANOTHER voice is a bus program (FR_STREAM_BUS), refused without the option with the mix-bus text;
  * `lookback` is at least the largest amount the patch can ask for: base + depth, or the 48 of Minimum(In(1), 48);
  * a signal delay inside a loop program, of an input row, or with a bound observed from input rows stays refused.

The oracle evaluates a Delay by evaluating its source again, so a row costs (voice evaluations per frame) x (partials) leaf
evaluations per frame: a chorus row 2, each constant tap behind it twice as many, a comb as stream_loop_cases counts it.  The
comparison with the oracle covers the leading frames that stay within stream_general_cases.ORACLE_LEAF_BUDGET; the comparison
with fr_fill_buffer covers every sample."""
import numpy as np

import stream_general_cases as G
import stream_loop_cases as L
from libfriendship_amd import synth
from stream_general_cases import IDLE, blocks_of, block_rows, fill_compare, short_blocks, silence_voice, stream_all   # noqa: F401  (the tests take them from here)
from stream_loop_cases import oracle_frames

NEW_KERNEL = "bank_stream_dyn_kernel"
NEW_KEYS = ("dyn_reads", "dyn_steps", "lookback")
PROGRAMS = dict(G.PROGRAMS)                                     # FR_STREAM_PROGRAMS alone
OPTION = dict(PROGRAMS, FR_STREAM_DYN="1")
INPUTS = dict(OPTION, FR_STREAM_INPUTS="1")
BUS = dict(OPTION, FR_STREAM_BUS="1")
GENERAL = dict(OPTION, FR_STREAM_GENERAL="1")
LOOPS = dict(OPTION, FR_STREAM_LOOPS="1")
OBSERVED = dict(INPUTS, FR_DELAY_OBSERVED="1")
OLD_REASON = "a program uses S_READ_DYN (a Delay by a signal amount), which block streaming does not serve yet"
KNOB_BOUND = 48
KNOB_SCALE = np.float32(40.0)                                   # control rows are within +-1.5: amounts within +-60


def _voices(g, V, P, seed=0x5EED0A00):
    p = synth.voice_params(V, P, seed, wrap=64)
    return synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P))


def _to_rows(g, roots):
    roots = np.asarray(roots, dtype=np.uint32)
    g.edge(roots, 0, 0, np.arange(len(roots), dtype=np.uint32))
    return g.finish(len(roots))


def _lfo_amount(g, lo=1.0, depth=30.0):
    """lo + depth * Modulo(t * 0.001, 1): lo .. lo + depth frames (stream_loop_cases.dyn_loop_tree's amount)."""
    f = np.float32
    lfo = g.binop(synth.K_MOD, g.binop(synth.K_MUL, synth.IN(0), synth.C(f(0.001)), 1), synth.C(f(1.0)), 1)
    return g.binop(synth.K_SUM2, synth.C(f(lo)), g.binop(synth.K_MUL, synth.C(f(depth)), lfo, 1), 1)


def _knob_amount(g):
    """Minimum(In(1), 48): whatever the control row holds, at most 48 frames."""
    return g.binop(synth.K_MIN, synth.IN(1), synth.C(np.float32(KNOB_BOUND)), 1)


def _delay(g, src, amount, n):
    """Delay(src, amount): src a handle array or a constant, amount one node for all."""
    return g.binop(synth.K_DELAY, src, np.broadcast_to(amount, (n,)), n)


def dry_tree(V, P):
    """Row v = voice v of the patches below, nothing behind it."""
    g = synth.GraphArrays()
    return _to_rows(g, _voices(g, V, P))


def knob_tree(V, P):
    """Row v = voice v + Delay(voice v, Minimum(In(1), 48)): the delay time on a knob."""
    g = synth.GraphArrays()
    v = _voices(g, V, P)
    return _to_rows(g, g.binop(synth.K_SUM2, v, _delay(g, v, _knob_amount(g), V), V))


def step_knob_tree(V, P):
    """Row v = voice v + Delay(C(0.75), Minimum(In(1), 48)): a signal Delay of a constant (S_STEP_DYN)."""
    g = synth.GraphArrays()
    v = _voices(g, V, P)
    step = g.nodes(synth.K_DELAY, 1)
    g.const(step, np.float32(0.75), 0)
    g.edge(_knob_amount(g), step, 0, 1)
    return _to_rows(g, g.binop(synth.K_SUM2, v, np.broadcast_to(step, (V,)), V))


def cross_tree(V, P):
    """Row v = voice v + Delay(voice (v + 1) mod V, 1 + 30 * Modulo(t * 0.001, 1)): the delayed voice is another one's."""
    g = synth.GraphArrays()
    v = _voices(g, V, P)
    return _to_rows(g, g.binop(synth.K_SUM2, v, _delay(g, np.roll(v, -1), _lfo_amount(g), V), V))


def beside_loop_tree(V, P):
    """Rows 0 .. V-1: x = voice v + 0.6 * Delay(x, 5); rows V .. 2V-1: voice v + 0.25 * Delay(voice v, 1 + 30 * lfo)."""
    g = synth.GraphArrays()
    v = _voices(g, V, P)
    x = L._loop(g, v, [(5, 0.6)], V)
    wet = g.binop(synth.K_MUL, _delay(g, v, _lfo_amount(g), V), synth.C(np.float32(0.25)), V)
    return _to_rows(g, np.concatenate([x, g.binop(synth.K_SUM2, v, wet, V)]))


def delayed_input_tree(V, P):
    """Row v = voice v + Delay(In(1), 1 + 30 * lfo): a signal delay of an input row (S_READ_INPUT_DYN)."""
    g = synth.GraphArrays()
    v = _voices(g, V, P)
    dl = g.nodes(synth.K_DELAY, 1)
    g.edge(0, dl, 1, 0)
    g.edge(_lfo_amount(g), dl, 0, 1)
    return _to_rows(g, g.binop(synth.K_SUM2, v, np.broadcast_to(dl, (V,)), V))


def observed_tree(V, P):
    """Row v = voice v + Delay(voice v, 100 + 300 * In(1)): the bound exists only as an observation of the rows of In(1)."""
    g = synth.GraphArrays()
    f = np.float32
    v = _voices(g, V, P)
    amt = g.binop(synth.K_SUM2, synth.C(f(100.0)), g.binop(synth.K_MUL, synth.C(f(300.0)), synth.IN(1), 1), 1)
    return _to_rows(g, g.binop(synth.K_SUM2, v, _delay(g, v, amt, V), V))


def _case(name, build, n_rows, options, bound, reads, steps=0, per_voice=None, bus=0, n_in=1, P=128, V=2, evals=2, loop=None, leaves=None, strides=()):
    """bound: the largest amount in frames with which a ring is read; reads / steps: dyn_reads / dyn_steps; per_voice: programs_per_voice, sorted;
    evals: voice evaluations per frame of all rows together (the oracle's cost); loop: the taps of a loop that `evals` does not
    count, each of its rows having a quarter of the budget; leaves: general_voices (FR_STREAM_GENERAL)."""
    frames = G.ORACLE_LEAF_BUDGET // (P * evals)
    if loop:
        frames = min(frames, oracle_frames(loop, G.ORACLE_LEAF_BUDGET // P // 4))
    return {"name": name, "build": build, "n_rows": n_rows, "options": options, "bound": bound, "reads": reads, "steps": steps, "voices": V,
            "per_voice": sorted(per_voice if per_voice is not None else [1] * V), "bus": bus, "n_in": n_in, "oracle_frames": frames, "P": P,
            "leaves": leaves, "strides": list(strides)}


SERVABLE = [
    # amounts 400..700: every read lands in earlier blocks; the bound sizes the rings and the warm-up
    _case("chorus_2x128", lambda: synth.chorus_tree(2, 128), 2, OPTION, 700, 2, evals=4),
    # 3..23 frames: reads of the frames the wave has just stored, and across the block boundary
    _case("chorus_short", lambda: synth.chorus_tree(2, 128, depth=20.0, base=3.0), 2, OPTION, 23, 2, evals=4),
    # amount 0 (the same frame), the floor, and frame < frames => 0.0 on the first frames from 0
    _case("chorus_zero", lambda: synth.chorus_tree(2, 128, depth=5.0, base=0.0), 2, OPTION, 5, 2, evals=4),
    # the fused form: S_STORE, constant reads >= 64 of program rings next to the signal read (every tap doubles the oracle's cost)
    _case("chorus_taps", lambda: synth.chorus_tree(2, 128, depth=20.0, base=3.0, taps=2, base_delay=100.0), 2, OPTION, 23, 2, evals=16),
    _case("knob", lambda: knob_tree(2, 128), 2, INPUTS, KNOB_BOUND, 2, n_in=2, evals=4),
    # (S_STEP_DYN touches no memory: no ring has to look back for it)
    _case("step_knob", lambda: step_knob_tree(2, 128), 2, INPUTS, 0, 0, steps=2, n_in=2, evals=2),
    # a signal read of another voice makes a bus program
    _case("cross_3", lambda: cross_tree(3, 128), 3, BUS, 31, 3, per_voice=[0, 0, 0], bus=3, V=3, evals=6),
    # schedule banks in the new kernel (the cases above have none)
    _case("chorus_2x100", lambda: synth.chorus_tree(2, 100, depth=20.0, base=3.0), 2, GENERAL, 23, 2, P=100, evals=4, leaves=[100, 100]),
    # loop programs and signal-delay programs of one voice in one launch
    _case("beside_loop", lambda: beside_loop_tree(2, 128), 4, LOOPS, 31, 2, per_voice=[2, 2], evals=4, loop=(5,), strides=[5, 5]),
]

# (name, builder, output rows, options, input rows, fragments of the reason with FR_STREAM_DYN on)
REFUSED = [
    ("dyn_in_loop", lambda: L.dyn_loop_tree(2, 128), 2, LOOPS, 1, ("a loop program uses S_READ_DYN", "inside a feedback loop shorter than a block")),
    ("cross_3_without_bus", lambda: cross_tree(3, 128), 3, OPTION, 1, ("in the same block (a mix bus across voices); each streamed program follows one voice",)),
    ("delayed_input", lambda: delayed_input_tree(2, 128), 2, INPUTS, 2, ("S_READ_INPUT_DYN (a delayed read of an input row)", "a stream keeps no input history")),
    ("observed_bound", lambda: observed_tree(2, 128), 2, OBSERVED, 2, ("a Delay's bound was observed from input rows (FR_DELAY_OBSERVED)",)),
]


def case(name):
    for c in SERVABLE:
        if c["name"] == name:
            return c
    raise KeyError(name)


def knob_blocks(blocks):
    """blocks_of's blocks with the control rows scaled to amounts: negative, fractional, above the knob's 48, and the hostile
    values (+-0, denormals, +-inf, NaN) as they are."""
    with np.errstate(invalid="ignore", over="ignore"):
        return [(idx, T, [rows[0]] + [(r * KNOB_SCALE).astype(np.float32) for r in rows[1:]]) for idx, T, rows in blocks]


def check_stream_object(s, c):
    """fr_plan_json["stream"] of a servable case against the graph's expectations."""
    assert s["servable"] is True and s["reason"] == "", s
    assert s["kernel"] == NEW_KERNEL, s
    assert s["dyn_reads"] == c["reads"] and s["dyn_steps"] == c["steps"], s
    assert s["voices"] == c["voices"], s
    assert sorted(s["programs_per_voice"]) == c["per_voice"] and s["bus_programs"] == c["bus"], s
    assert len(s["input_slots"]) == c["n_in"] and s["input_slots"] == list(range(c["n_in"])), s
    assert s["lookback"] >= c["bound"], s
    if c["leaves"] is not None:
        assert s["general_voices"] == c["leaves"], s
    if c["strides"]:
        assert sorted(l for l in s["loop_programs"] if l) == c["strides"], s
