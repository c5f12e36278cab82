"""Patches for block streaming of delayed reads of input rows (FR_STREAM_HISTORY on top of FR_STREAM_PROGRAMS), shared by the
simulator tests of the serving rule (tests/test_stream_hist_sim.py) and the GPU tests of the resident kernel
(tests/test_hip_stream_hist.py).  Graph recipes and plain data: importable without a GPU.

Delay(In(k), d) -- a pre-delay on a control row, a delayed gate, the time row itself read late -- is S_READ_INPUT in the program
of every row that uses it (with a signal amount and FR_STREAM_DYN: S_READ_INPUT_DYN); the stream keeps a history of the rows it
is fed.  Voices are 2 x 128 partials, the smallest the chunked kernels serve.  Expectations come from the graph:
  * a row that is one voice combined with a delayed input is ONE program of that voice; every Delay of an input the row's
    expression holds is one read of that program (`reads`: hist_reads, `dyn_reads`: hist_dyn_reads, over all programs);
  * `lookback` (input_lookback) is the largest constant amount; of a signal amount the largest value it can take, floored: 31
    for 1 + 30 * Modulo(t * 0.001, 1) (f32 rounding can reach 31.0), 48 for Minimum(In(2), 48);
  * `input_slots` is slot 0 followed by every other slot read, delayed or not;
  * a row that needs two voices of the block is a bus program (FR_STREAM_BUS); a read inside a loop (FR_STREAM_LOOPS) is one
    more frame-only load of the loop program, which keeps the comb's stride.

A case's sequence is two streams on one renderer.  The first has 12 blocks in three segments: from frame 0 (the lengths of
stream_cases.FIRST_LENGTHS and a last block of 5 frames: 300 frames, so a history of 256 frames -- d = 100 -- wraps in it), a
seek forward to frame 5003 and a seek back to frame 69, each a full block and a short last one; the second, after fr_stream_end
and fr_stream_begin, starts at frame 0 again.  Time rows are stream_cases.finite_block_rows (hostile finite values in every fifth
block, +-inf and NaN in a segment's last block, which is short here: a delayed NaN is a NaN d frames later); control rows are
stream_loop_cases.blocks_of through stream_matrix.finite_controls."""
import zlib

import numpy as np

import stream_cases as K
import stream_dyn_cases as D
import stream_general_cases as G
import stream_input_cases as I
import stream_loop_cases as L
import stream_matrix as X
from libfriendship_amd import synth

NEW_KERNEL = "bank_stream_hist_kernel"
NEW_KEYS = ("hist_reads", "hist_dyn_reads", "input_lookback")
PROGRAMS = dict(K.OPTION)                                       # FR_STREAM_PROGRAMS alone
OPTION = dict(PROGRAMS, FR_STREAM_HISTORY="1")
INPUTS = dict(OPTION, FR_STREAM_INPUTS="1")
BUS = dict(INPUTS, FR_STREAM_BUS="1")
LOOPS = dict(INPUTS, FR_STREAM_LOOPS="1")
DYN = dict(INPUTS, FR_STREAM_DYN="1")
OBSERVED = dict(DYN, FR_DELAY_OBSERVED="1")
IDLE = dict(L.IDLE)
HIST_MAX_FRAMES = 1 << 20                                       # csrc/streamplan.hpp STREAM_HIST_MAX_FRAMES
FINITE_SHARE = 0.95
SENSITIVITY = 0.90                                              # share of a fed row's finite samples that one more frame of delay must change
STREAMS = [[(0, 300), (5003, 68), (69, 70)], [(0, 134)]]
SLOT_DELAYS = (3, 1, 64, 17, 100, 63, 2, 130)                   # all eight slots, each at its own delay


def _voices(g, V, P, seed=0x5EED0C00):
    return D._voices(g, V, P, seed)


def _delayed_input(g, slot, d):
    """Delay(In(slot), d), one node."""
    dl = g.nodes(synth.K_DELAY, 1)
    g.edge(0, dl, slot, 0)
    g.const(dl, np.float32(d), 1)
    return dl


def time_delay_tree(V, P, d=7.0):
    """Row v = voice_v + Delay(In(0), d): the time row itself, read d frames late."""
    g = synth.GraphArrays()
    v = _voices(g, V, P)
    return D._to_rows(g, g.binop(synth.K_SUM2, v, np.broadcast_to(_delayed_input(g, 0, d), (V,)), V))


def slots_tree(V, P, delays=SLOT_DELAYS):
    """Row v = voice_v * (Delay(In(0), d0) * 2^-20 + Delay(In(1), d1) + ... ): every slot at its own delay."""
    g = synth.GraphArrays()
    ctl = g.binop(synth.K_MUL, _delayed_input(g, 0, delays[0]), synth.C(np.float32(2.0 ** -20)), 1)
    for s in range(1, len(delays)):
        ctl = g.binop(synth.K_SUM2, ctl, _delayed_input(g, s, delays[s]), 1)
    v = _voices(g, V, P)
    return D._to_rows(g, g.binop(synth.K_MUL, v, np.broadcast_to(ctl, (V,)), V))


def bus_tree(V, P, d=30.0):
    """One row: (0.5 * voice_0 + 0.25 * voice_1 + ...) * Delay(In(1), d).  (The gains keep the matcher from folding the voices into one.)"""
    g = synth.GraphArrays()
    v = _voices(g, V, P)
    terms = [g.binop(synth.K_MUL, v[k:k + 1], synth.C(np.float32(0.5 ** (k + 1))), 1) for k in range(V)]
    bus = terms[0]
    for t in terms[1:]:
        bus = g.binop(synth.K_SUM2, bus, t, 1)
    return D._to_rows(g, g.binop(synth.K_MUL, bus, _delayed_input(g, 1, d), 1))


def loop_tree(V, P, d_in=3.0, taps=((5, 0.6),)):
    """x = (voice + Delay(In(1), d_in)) + 0.6 * Delay(x, 5): the delayed read inside the comb's loop."""
    g = synth.GraphArrays()
    v = _voices(g, V, P)
    src = g.binop(synth.K_SUM2, v, np.broadcast_to(_delayed_input(g, 1, d_in), (V,)), V)
    x = L._loop(g, src, list(taps), V)
    return D._to_rows(g, x)


def knob_input_tree(V, P):
    """Row v = voice_v + Delay(In(1), Minimum(In(2), 48)): an input row delayed by a knob."""
    g = synth.GraphArrays()
    v = _voices(g, V, P)
    return D._to_rows(g, g.binop(synth.K_SUM2, v, np.broadcast_to(_knob_delayed_input(g), (V,)), V))


def _knob_delayed_input(g):
    """Delay(In(1), Minimum(In(2), 48)), one node."""
    amount = g.binop(synth.K_MIN, synth.IN(2), synth.C(np.float32(D.KNOB_BOUND)), 1)
    dl = g.nodes(synth.K_DELAY, 1)
    g.edge(0, dl, 1, 0)
    g.edge(amount, dl, 0, 1)
    return dl


def observed_tree(V, P):
    """Row v = Delay(voice_v, 100 + 300 * In(2)) + Delay(In(1), Minimum(In(2), 48)): the voice's bound exists only as an
    observation of the rows of In(2) (stream_dyn_cases.observed_tree), next to a delayed input with a proven one."""
    g = synth.GraphArrays()
    f = np.float32
    v = _voices(g, V, P)
    amount = g.binop(synth.K_SUM2, synth.C(f(100.0)), g.binop(synth.K_MUL, synth.C(f(300.0)), synth.IN(2), 1), 1)
    return D._to_rows(g, g.binop(synth.K_SUM2, D._delay(g, v, amount, V), np.broadcast_to(_knob_delayed_input(g), (V,)), V))


def unbounded_tree(V, P):
    """Row v = voice_v + Delay(In(1), 100 + 300 * In(2)): an input delayed by an amount nobody can bound."""
    g = synth.GraphArrays()
    f = np.float32
    v = _voices(g, V, P)
    amount = g.binop(synth.K_SUM2, synth.C(f(100.0)), g.binop(synth.K_MUL, synth.C(f(300.0)), synth.IN(2), 1), 1)
    dl = g.nodes(synth.K_DELAY, 1)
    g.edge(0, dl, 1, 0)
    g.edge(amount, dl, 0, 1)
    return D._to_rows(g, g.binop(synth.K_SUM2, v, np.broadcast_to(dl, (V,)), V))


def dyn_in_loop_tree(V, P):
    """x = (voice + Delay(In(1), 1 + 30 * lfo)) + 0.6 * Delay(x, 5): a signal delay of an input row inside a loop program."""
    g = synth.GraphArrays()
    v = _voices(g, V, P)
    dl = g.nodes(synth.K_DELAY, 1)
    g.edge(0, dl, 1, 0)
    g.edge(D._lfo_amount(g), dl, 0, 1)
    src = g.binop(synth.K_SUM2, v, np.broadcast_to(dl, (V,)), V)
    return D._to_rows(g, L._loop(g, src, [(5, 0.6)], V))


def nine_slots_tree(V, P):
    return slots_tree(V, P, SLOT_DELAYS + (5,))


def _case(name, build, n_rows, options, lookback, reads=0, dyn_reads=0, per_voice=(1, 1), bus=0, n_in=2, evals=1, loop=None, strides=(), knob=False,
          semantics="reference", delay_rows=None):
    """lookback: input_lookback; reads / dyn_reads: hist_reads / hist_dyn_reads; evals: voice evaluations per frame of all rows
    together (the oracle's cost); loop: the taps of the patch's loop, which `evals` does not count."""
    frames = G.ORACLE_LEAF_BUDGET // (128 * evals)
    if loop:
        frames = min(frames, L.oracle_frames(loop, G.ORACLE_LEAF_BUDGET // 128 // 2))
    return {"name": name, "build": build, "n_rows": n_rows, "options": options, "lookback": lookback, "reads": reads, "dyn_reads": dyn_reads, "voices": 2,
            "per_voice": sorted(per_voice), "bus": bus, "n_in": n_in, "oracle_frames": min(frames, STREAMS[0][0][1]), "strides": list(strides), "knob": knob,
            "semantics": semantics, "delay_rows": list(range(n_rows)) if delay_rows is None else list(delay_rows), "streams": STREAMS}


SERVABLE = [_case(f"gate_{d}", (lambda d=d: I.delayed_input_tree(2, 128, float(d))), 2, INPUTS, d, reads=2, evals=2) for d in (1, 63, 64, 65, 100)] + [
    # the time row delayed: a one-row history, no FR_STREAM_INPUTS needed
    _case("time_7", lambda: time_delay_tree(2, 128), 2, OPTION, 7, reads=2, n_in=1, evals=2),
    _case("eight_slots", lambda: slots_tree(2, 128), 2, INPUTS, max(SLOT_DELAYS), reads=16, n_in=8, evals=2),
    _case("bus_30", lambda: bus_tree(2, 128), 1, BUS, 30, reads=1, per_voice=(0, 0), bus=1, evals=2),
    # one loop program per voice: the voice's ring, the delayed input and the own read are its three loads
    _case("comb_5_in_3", lambda: loop_tree(2, 128), 2, LOOPS, 3, reads=2, loop=(5,), strides=[5, 5]),
    _case("comb_5_in_3_sparkle", lambda: loop_tree(2, 128), 2, LOOPS, 3, reads=2, loop=(5,), strides=[5, 5], semantics="sparkle"),
    _case("lfo_input", lambda: D.delayed_input_tree(2, 128), 2, DYN, 31, dyn_reads=2, evals=2, delay_rows=()),
    _case("knob_input", lambda: knob_input_tree(2, 128), 2, DYN, D.KNOB_BOUND, dyn_reads=2, n_in=3, evals=2, knob=True, delay_rows=()),
    _case("knob_input_sparkle", lambda: knob_input_tree(2, 128), 2, DYN, D.KNOB_BOUND, dyn_reads=2, n_in=3, evals=2, knob=True, delay_rows=(), semantics="sparkle"),
]

OLD_INPUT = "a program uses S_READ_INPUT (a delayed read of the input row), which block streaming does not serve yet"
OLD_INPUT_DYN = "a program uses S_READ_INPUT_DYN (a delayed read of an input row), which block streaming does not serve yet: a stream keeps no input history"

# (name, builder, output rows, options, input rows, fragments of the reason)
REFUSED = [
    # the option off: both old texts, word for word
    ("off_constant", lambda: I.delayed_input_tree(2, 128, 100.0), 2, dict(PROGRAMS, FR_STREAM_INPUTS="1"), 2, (OLD_INPUT,)),
    ("off_signal", lambda: D.delayed_input_tree(2, 128), 2, D.INPUTS, 2, (OLD_INPUT_DYN,)),
    # a signal amount without FR_STREAM_DYN: refused as a Delay by a signal amount, with that text
    ("signal_without_dyn", lambda: D.delayed_input_tree(2, 128), 2, INPUTS, 2,
     ("a program uses S_READ_INPUT_DYN (a Delay by a signal amount), which block streaming does not serve yet",)),
    ("slot_1_without_inputs", lambda: I.delayed_input_tree(2, 128, 100.0), 2, OPTION, 2, ("a program reads input slot 1; block streaming feeds slot 0 only",)),
    ("observed_bound", lambda: observed_tree(2, 128), 2, OBSERVED, 3, ("a Delay's bound was observed from input rows (FR_DELAY_OBSERVED)",)),
    ("no_proven_bound", lambda: unbounded_tree(2, 128), 2, DYN, 3, ("delays an input row by a signal amount without a proven bound",)),
    ("dyn_in_loop", lambda: dyn_in_loop_tree(2, 128), 2, dict(DYN, FR_STREAM_LOOPS="1"), 2,
     ("a loop program uses S_READ_INPUT_DYN", "inside a feedback loop shorter than a block")),
    ("lookback_over_the_limit", lambda: I.delayed_input_tree(2, 128, float(HIST_MAX_FRAMES + 1)), 2, INPUTS, 2,
     (f"reads an input row {HIST_MAX_FRAMES + 1} frames back", f"holds at most {HIST_MAX_FRAMES} frames")),
    ("nine_slots", lambda: nine_slots_tree(2, 128), 2, INPUTS, 9, ("9 distinct input slots (slot 0 included); block streaming feeds at most 8",)),
    # 31 own reads and the voice's ring are 32 loads (stream_loop_cases.many_reads_tree); the delayed input is the 33rd
    ("loop_loads_count_the_read", lambda: loop_tree(2, 128, taps=tuple((k + 1, 2.0 ** -(k + 2)) for k in range(L.LOOP_LOADS - 1))), 2, LOOPS, 2,
     (f"a loop program has {L.LOOP_LOADS + 1} frame-only loads; block streaming serves at most {L.LOOP_LOADS}",)),
]


def case(name):
    for c in SERVABLE:
        if c["name"] == name:
            return c
    raise KeyError(name)


class _FullBlocks:
    """stream_cases.finite_block_rows asks its generator for the length of every block after the first seven: full blocks here.
    Everything else it draws -- where the hostile values go -- comes from the generator."""

    def __init__(self, rng):
        self.rng = rng

    def integers(self, low, high=None, size=None):
        if (low, high, size) == (1, 65, None):
            return 64
        return self.rng.integers(low, high, size=size)


def knob_controls(blocks):
    """The amount's row (slot 2) scaled to frames -- negative, fractional, 0, beyond the knob's 48 -- and with +-inf and NaN in
    every second block, as stream_loop_cases.blocks_of made them: an amount that is no number delays by 0 frames (sparkle: the
    row reads 0.0) and leaves the output finite.  The delayed row (slot 1) stays as finite_controls left it."""
    return [(idx, T, [rows[0], rows[1], (rows[2] * D.KNOB_SCALE).astype(np.float32)]) for idx, T, rows in blocks]


def streams_of(c):
    """The case's streams: [[(idx, T, rows)]], the control rows from a generator seeded by the case's name."""
    rng_t, rng = np.random.default_rng(0x415), np.random.default_rng(zlib.crc32(c["name"].split("_sparkle")[0].encode()))
    out = []
    for starts in c["streams"]:
        raw = L.blocks_of(K.finite_block_rows(_FullBlocks(rng_t), starts), rng, c["n_in"])
        blocks = X.finite_controls(raw)
        if c["knob"]:
            with np.errstate(invalid="ignore", over="ignore"):
                blocks = knob_controls([(idx, T, [b[0], b[1], r[2]]) for (idx, T, b), (_, _, r) in zip(blocks, raw)])
        out.append(blocks)
    return out


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


def check_stream_object(s, c):
    """fr_plan_json["stream"] of a servable case against the graph's expectations."""
    assert s["servable"] is True and s["reason"] == "", s
    assert s["kernel"] == NEW_KERNEL, s
    assert s["hist_reads"] == c["reads"] and s["hist_dyn_reads"] == c["dyn_reads"] and s["input_lookback"] == c["lookback"], s
    assert s["voices"] == c["voices"], s
    assert sorted(s["programs_per_voice"]) == c["per_voice"] and s["bus_programs"] == c["bus"], s
    assert s["input_slots"] == list(range(c["n_in"])), s
    if c["strides"]:
        assert sorted(l for l in s["loop_programs"] if l) == c["strides"], s


# ---- the store's rules through the history (tests/test_hip_stream_hist.py) ------------------------------------------------------

def store_rule_blocks(rng, d):
    """(blocks as they are fed, blocks as streamrows.hpp says slot 1 reads them): eight full blocks from frame 0 in which slot 1
    gets a full row, a SHORT row (padded with its own last value), an EMPTY row after a fed one (the slot's last value), the
    three again, and in the last two blocks NO row (+0.0; a slot left out cannot be fed again, so these come last)."""
    g = lambda n: rng.uniform(0.5, 1.5, size=n).astype(np.float32)
    t = synth.time_ramp
    fed, read, idx, last = [], [], 0, np.float32(0.0)
    for kind in ("full", "short", "empty", "full", "short", "empty", "none", "none"):
        T = 64
        row = {"full": g(T), "short": g(17), "empty": np.zeros(0, np.float32), "none": None}[kind]
        if row is None:
            fed.append((idx, T, [t(idx, idx + T)]))
            read.append((idx, T, [t(idx, idx + T), np.zeros(T, np.float32)]))
        else:
            fed.append((idx, T, [t(idx, idx + T), row]))
            full = I.padded(row, T, last)
            read.append((idx, T, [t(idx, idx + T), full]))
            last = full[-1]
        idx += T
    assert idx > d + 3 * 64
    return fed, read
