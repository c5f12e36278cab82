"""Patches WITHOUT A VOICE for block streaming (FR_STREAM_EFFECTS on top of FR_STREAM_PROGRAMS), shared by the simulator tests of
the serving rule (tests/test_stream_fx_sim.py) and the GPU tests of the resident kernel (tests/test_hip_stream_fx.py).  Graph
recipes and plain data: importable without a GPU.

Such a patch has no oscillator bank at all: an echo, a comb or a flanger on a row the host feeds in, a gain or a minimum of two
control rows, a one-pole smoother on a knob.  Its stage programs are dealt over SEGMENTS, one workgroup of one wave each
(csrc/streamplan.hpp): every program gets a group in the order the programs run, a program that reads an earlier program's ring
less than a block back -- or copies it to a row -- follows that program's group, one that would follow two groups is a bus
program, and group g runs in segment g % segments.  Expectations come from the graph:
  * `segments`: the groups, at most the device's workgroups (`rows_260`: more rows than any device has CUs, so the number is
    min(260, max_workgroups) and the groups wrap); `per_segment`: the programs of each segment, sorted; `bus`: the bus programs;
  * `strides`: the stride of every loop program (a delay below a block), sorted;
  * `reads` / `lookback`: the delayed reads of input rows (hist_reads) and the deepest of them (input_lookback);
  * `n_in`: the input slots the patch reads, slot 0 included whether or not a program reads it: it stays row 0 of every block.

A case's sequence is stream_hist_cases.STREAMS: two streams on one renderer, 12 blocks with a seek forward to frame 5003 and a
seek back to frame 69, then a second stream from frame 0.  Time rows are stream_cases.finite_block_rows, control rows go through
stream_matrix.finite_controls (stream_hist_cases.streams_of), loop gains are below 1 in magnitude."""
import numpy as np

import stream_hist_cases as H
import stream_loop_cases as L
from libfriendship_amd import synth

NEW_KERNEL = "bank_stream_fx_kernel"
NEW_KEYS = ("segments",)
PROGRAMS = dict(H.PROGRAMS)                                     # FR_STREAM_PROGRAMS alone
OPTION = dict(PROGRAMS, FR_STREAM_EFFECTS="1")
INPUTS = dict(OPTION, FR_STREAM_INPUTS="1")
LOOPS = dict(INPUTS, FR_STREAM_LOOPS="1")
HISTORY = dict(INPUTS, FR_STREAM_HISTORY="1")
IDLE = dict(L.IDLE)
FINITE_SHARE = H.FINITE_SHARE
SENSITIVITY = H.SENSITIVITY
STREAMS = H.STREAMS
MAX_WGS = 256                                                   # csrc/streamplan.hpp STREAM_MAX_WGS
OLD_REASON = "block streaming needs a plan with one voice bank (this one: 0 bank launches)"
NO_FUSED_FORM = "the plan has no fused form: a program's ring is read less than 64 frames back (or the fused programs exceed the interpreter's budget)"
DYN_OF_A_PROGRAM = ("a program uses S_READ_DYN of a ring that a program stores (a Delay of a computed value by a signal amount, which may be 0 "
                    "frames); block streaming serves signal delays of voices only")
TINY = np.float32(2.0 ** -20)                                   # the time row reaches 2^32: scaled to the control rows' size


def _rows(g, roots):
    roots = np.asarray(roots, dtype=np.uint32)
    g.edge(roots, 0, 0, np.arange(len(roots), dtype=np.uint32))
    return g.finish(len(roots))


def _delay(g, src, d):
    """Delay(src, d): src a handle array or synth.IN(slot)."""
    return g.binop(synth.K_DELAY, src, synth.C(np.float32(d)), 1)


def _loop_on(g, src, d, gain):
    """x = src + gain * Delay(x, d): src a handle array or synth.IN(slot)."""
    dl = g.nodes(synth.K_DELAY, 1)
    g.const(dl, np.float32(d), 1)
    x = g.binop(synth.K_SUM2, src, g.binop(synth.K_MUL, dl, synth.C(np.float32(gain)), 1), 1)
    g.edge(x, dl, 0, 0)
    return x


def gain_tree():
    """row0 = In(0) * 2^-20."""
    g = synth.GraphArrays()
    return _rows(g, g.binop(synth.K_MUL, synth.IN(0), synth.C(TINY), 1))


def pass_const_tree():
    """row0 = In(1), row1 = the constant 0.25: the output's edges come straight from the input and from the constant node."""
    g = synth.GraphArrays()
    g.edge(0, 0, 1, 0)
    g.const(0, np.float32(0.25), 1)
    return g.finish(2)


def two_rows_tree():
    """row0 = In(0) * 2^-20 * In(1); row1 = Minimum(In(1), In(2))."""
    g = synth.GraphArrays()
    a = g.binop(synth.K_MUL, g.binop(synth.K_MUL, synth.IN(0), synth.C(TINY), 1), synth.IN(1), 1)
    b = g.binop(synth.K_MIN, synth.IN(1), synth.IN(2), 1)
    return _rows(g, np.concatenate([a, b]))


def echo_tree(d, gain=0.5):
    """x = In(1) + 0.5 * Delay(x, d): an echo (d >= 64), a comb, a one-pole (d = 1)."""
    g = synth.GraphArrays()
    return _rows(g, _loop_on(g, synth.IN(1), d, gain))


def fir_tree():
    """In(1) + 0.5 * Delay(In(1), 1) + 0.25 * Delay(In(1), 64) + 0.125 * Delay(In(1), 100)."""
    g = synth.GraphArrays()
    acc = None
    for d, c in ((1, 0.5), (64, 0.25), (100, 0.125)):
        term = g.binop(synth.K_MUL, _delay(g, synth.IN(1), d), synth.C(np.float32(c)), 1)
        acc = g.binop(synth.K_SUM2, synth.IN(1) if acc is None else acc, term, 1)
    return _rows(g, acc)


def flanger_tree():
    """In(1) + Delay(In(1), Minimum(In(2), 48))."""
    g = synth.GraphArrays()
    return _rows(g, g.binop(synth.K_SUM2, synth.IN(1), H._knob_delayed_input(g), 1))


def comb_delayed_in_tree():
    """x = Delay(In(1), 3) + 0.6 * Delay(x, 5)."""
    g = synth.GraphArrays()
    return _rows(g, _loop_on(g, _delay(g, synth.IN(1), 3), 5, 0.6))


def tap_behind_tree():
    """row0 = x = In(1) + 0.6 * Delay(x, 3); row1 = Delay(x, 2) * In(2)."""
    g = synth.GraphArrays()
    x = _loop_on(g, synth.IN(1), 3, 0.6)
    return _rows(g, np.concatenate([x, g.binop(synth.K_MUL, _delay(g, x, 2), synth.IN(2), 1)]))


def bus_of_combs_tree():
    """row0 = x = In(1) + 0.6 * Delay(x, 3); row1 = y = In(2) - 0.5 * Delay(y, 4); row2 = Delay(x, 1) + Delay(y, 2)."""
    g = synth.GraphArrays()
    x, y = _loop_on(g, synth.IN(1), 3, 0.6), _loop_on(g, synth.IN(2), 4, -0.5)
    return _rows(g, np.concatenate([x, y, g.binop(synth.K_SUM2, _delay(g, x, 1), _delay(g, y, 2), 1)]))


N_MANY = 260
MANY_GAINS = (TINY * (np.float32(0.5) + np.arange(N_MANY, dtype=np.float32) / np.float32(N_MANY))).astype(np.float32)


def rows_260_tree():
    """row k = In(0) * c_k, 260 rows: more groups than a device has workgroups."""
    g = synth.GraphArrays()
    return _rows(g, g.binop(synth.K_MUL, synth.IN(0), synth.C(MANY_GAINS), N_MANY))


def product_delay_tree():
    """Delay(In(1) * In(2), 10): a feed-forward short delay of a program's ring."""
    g = synth.GraphArrays()
    return _rows(g, _delay(g, g.binop(synth.K_MUL, synth.IN(1), synth.IN(2), 1), 10))


def product_knob_delay_tree():
    """Delay(In(1) * In(2), Minimum(In(3), 48)): a signal delay of a program's ring."""
    g = synth.GraphArrays()
    amount = g.binop(synth.K_MIN, synth.IN(3), synth.C(np.float32(H.D.KNOB_BOUND)), 1)
    dl = g.nodes(synth.K_DELAY, 1)
    g.edge(g.binop(synth.K_MUL, synth.IN(1), synth.IN(2), 1), dl, 0, 0)
    g.edge(amount, dl, 0, 1)
    return _rows(g, dl)


def _case(name, build, n_rows, options, segments, per_segment, n_in, bus=0, strides=(), reads=0, lookback=0, knob=False, delay_rows=()):
    return {"name": name, "build": build, "n_rows": n_rows, "options": options, "segments": segments, "per_segment": sorted(per_segment), "bus": bus,
            "strides": sorted(strides), "reads": reads, "lookback": lookback, "n_in": n_in, "knob": knob, "semantics": "reference",
            "delay_rows": list(delay_rows), "oracle_frames": STREAMS[0][0][1], "streams": STREAMS}


SERVABLE = [
    _case("gain", gain_tree, 1, OPTION, 1, [1], 1),
    # (the planner makes a stage program of either row: a lone S_INPUT, a lone S_CONST)
    _case("pass_const", pass_const_tree, 2, INPUTS, 2, [1, 1], 2),
    _case("two_rows", two_rows_tree, 2, INPUTS, 2, [1, 1], 3),
    # a loop is ONE program: it stores its ring and writes its row
    _case("echo_100", lambda: echo_tree(100), 1, INPUTS, 1, [1], 2, delay_rows=[0]),
    _case("echo_64", lambda: echo_tree(64), 1, INPUTS, 1, [1], 2, delay_rows=[0]),
    _case("comb_5", lambda: echo_tree(5), 1, LOOPS, 1, [1], 2, strides=[5], delay_rows=[0]),
    _case("one_pole", lambda: echo_tree(1), 1, LOOPS, 1, [1], 2, strides=[1], delay_rows=[0]),
    _case("fir", fir_tree, 1, HISTORY, 1, [1], 2, reads=3, lookback=100, delay_rows=[0]),
    _case("flanger", flanger_tree, 1, dict(HISTORY, FR_STREAM_DYN="1"), 1, [1], 3, lookback=H.D.KNOB_BOUND, knob=True),
    _case("comb_delayed_in", comb_delayed_in_tree, 1, dict(HISTORY, FR_STREAM_LOOPS="1"), 1, [1], 2, strides=[5], reads=1, lookback=3, delay_rows=[0]),
    # the tap follows the comb's group: both in one segment
    _case("tap_behind", tap_behind_tree, 2, LOOPS, 1, [2], 3, strides=[3], delay_rows=[0, 1]),
    # the third row would follow both combs' groups: a bus program behind the two segments
    _case("bus_of_combs", bus_of_combs_tree, 3, dict(LOOPS, FR_STREAM_BUS="1"), 2, [1, 1], 3, bus=1, strides=[3, 4], delay_rows=[0, 1, 2]),
    _case("rows_260", rows_260_tree, N_MANY, OPTION, N_MANY, [1] * N_MANY, 1),
]


def without(options, *keys):
    return {k: v for k, v in options.items() if k not in keys}


# (name, builder, output rows, options, input rows, the reason, word for word)
REFUSED = [(f"{c['name']}_without_effects", c["build"], c["n_rows"], without(c["options"], "FR_STREAM_EFFECTS"), c["n_in"], OLD_REASON) for c in SERVABLE] + [
    ("bus_of_combs_without_bus", bus_of_combs_tree, 3, LOOPS, 3,
     "a program reads program groups 0 and 1 in the same block (a mix bus across program groups); each streamed program follows one program group"),
    ("product_delay", product_delay_tree, 1, dict(LOOPS, FR_STREAM_BUS="1", FR_STREAM_HISTORY="1", FR_STREAM_DYN="1"), 3, NO_FUSED_FORM),
    # (the planner cuts the product into a level of its own, so this patch has no fused form either and the rule says so before it
    # looks at an instruction; the sentence about S_READ_DYN of a ring that a program stores -- DYN_OF_A_PROGRAM -- is reached by the
    # hand-built one-level plan of tests/cpp/streamfx_tests.cpp)
    ("product_knob_delay", product_knob_delay_tree, 1, dict(LOOPS, FR_STREAM_BUS="1", FR_STREAM_HISTORY="1", FR_STREAM_DYN="1"), 4, NO_FUSED_FORM),
    ("fir_without_history", fir_tree, 1, INPUTS, 2, H.OLD_INPUT),
    ("comb_5_without_loops", lambda: echo_tree(5), 1, INPUTS, 2,
     "a program's ring is read 5 frames back; a streamed block needs delays of at least 64 frames"),
]


def case(name):
    for c in SERVABLE:
        if c["name"] == name:
            return c
    raise KeyError(name)


def refused(name):
    for r in REFUSED:
        if r[0] == name:
            return r
    raise KeyError(name)


def streams_of(c):
    """The case's streams, [[(idx, T, rows)]]: stream_hist_cases.streams_of with the case's name as the control rows' seed."""
    return H.streams_of(c)


_REFERENCES = {}


def reference_of(name):
    """(tree, streams, expected blocks per stream) of a case: the dense reference, rendered once per process and left unchanged."""
    if name not in _REFERENCES:
        import stream_reference
        c = case(name)
        tree, streams = c["build"](), streams_of(c)
        _REFERENCES[name] = (tree, streams, [stream_reference.expected_blocks(tree, blocks, c["semantics"]) for blocks in streams])
    return _REFERENCES[name]


def frames_of(c):
    return sum(n for starts in c["streams"] for _, n in starts)


def check_stream_object(s, c, max_wgs=MAX_WGS):
    """fr_plan_json["stream"] of a servable case against the graph's expectations.  `max_wgs`: the device's workgroups (the
    object's "max_workgroups" where FR_STREAM_BANKS reports it; the kernel's limit on the simulator, which knows no CU count)."""
    assert s["servable"] is True and s["reason"] == "", s
    assert s["kernel"] == NEW_KERNEL, s
    assert s["voices"] == 0 and s["chunks"] == 0, s
    segments = min(c["segments"], max_wgs)
    assert s["segments"] == segments, s
    per = c["per_segment"]
    if segments < c["segments"]:                                 # the groups wrap: group g runs in segment g % segments
        per = sorted(sum(per[g] for g in range(k, len(per), segments)) for k in range(segments))
    assert sorted(s["programs_per_voice"]) == per and s["bus_programs"] == c["bus"], s
    assert s["input_slots"] == list(range(c["n_in"])), s
    if "loop_programs" in s:
        assert sorted(l for l in s["loop_programs"] if l) == c["strides"], s
    else:
        assert not c["strides"]
    if "hist_reads" in s:
        assert s["hist_reads"] == c["reads"] and s["input_lookback"] == c["lookback"] and s["hist_dyn_reads"] == (1 if c["knob"] else 0), s
    else:
        assert c["reads"] == 0 and c["lookback"] == 0


# ---- the store's rules through an echo (tests/test_hip_stream_fx.py) ------------------------------------------------------------

def store_rule_blocks(rng):
    """stream_hist_cases.store_rule_blocks: slot 1 gets a full row, a short row, an empty row after a fed one, and at the end no
    row; what the echo of 100 frames repeats is what the slot read."""
    return H.store_rule_blocks(rng, 100)
