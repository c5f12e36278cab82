"""The case table of the streaming matrix: every resident kernel at its smallest plan, every (kernel, inherited feature) pair of
the cascade dyn > general > loops > banks > in > bus > prog, and one patch with all seven features, each with the sequence of
blocks it is streamed with.  Plain data and graph recipes, importable without a GPU; shared by tests/test_stream_matrix.py (the
dense reference of tests/stream_reference.py against the simulator's fr_fill_buffer and the oracle, the inputs' finite share,
the serving rule) and tests/test_hip_stream_matrix.py (the kernels against that reference, every sample).

A FEATURE is what fr_plan_json["stream"] shows (`features_of`): per-voice programs ("prog"), bus programs ("bus"), control rows
("in"), several banks ("banks"), loop programs ("loops"), schedule voices ("general"), Delays by a signal amount ("dyn").  The
kernel is the highest feature's; the others are INHERITED: 6 + 5 + 4 + 3 + 2 + 1 = 21 pairs.

A case's sequence is two streams on one renderer.  The first has three segments -- from frame 0, a seek forward to frame 5003
(no multiple of 64), a seek back to frame 69 --, the second, after fr_stream_end and fr_stream_begin, one segment from frame
269: it continues where the third ended, but a stream's first block is a seek.  Time rows are stream_cases.finite_block_rows
(hostile finite values on every fifth block, +-inf and NaN on a segment's last block, which a seek follows), control rows
stream_loop_cases.blocks_of (every second block with +-0, denormals, +-inf and NaN) through `finite_controls`, which keeps their
+-inf and NaN to a segment's last block too.  The first segment is 700 frames for a plan
with feedback and 1300 for a feed-forward one, whose rings hold 1024 frames and so wrap inside the stream.

`oracle_frames`: the leading frames of the first segment that the C++ oracle renders within the budget of the case's module
(it recurses without a memo: stream_loop_cases.oracle_frames, stream_general_cases.ORACLE_LEAF_BUDGET); a feed-forward patch of
these sizes it renders whole.  `delay_rows`: the output rows that a Delay of a constant amount feeds; `sensitivity`: the share of
their finite samples that must change when every such amount is raised by one frame."""
import zlib

import numpy as np

import stream_banks_cases as M
import stream_bus_cases as B
import stream_cases as K
import stream_dyn_cases as D
import stream_general_cases as G
import stream_input_cases as I
import stream_loop_cases as L
from libfriendship_amd import synth

KERNELS = ["prog", "bus", "in", "banks", "loops", "general", "dyn"]        # the cascade, lowest first: also the features' names
KERNEL_NAME = {"plain": "bank_stream_kernel", "prog": "bank_stream_prog_kernel", "bus": "bank_stream_bus_kernel", "in": I.NEW_KERNEL,
               "banks": M.NEW_KERNEL, "loops": L.NEW_KERNEL, "general": G.NEW_KERNEL, "dyn": D.NEW_KERNEL}
BY_PLAN = ("in", "banks", "loops", "general", "dyn")                      # fr_plan_json names these before any launch
PAIRS = [(k, f) for i, k in enumerate(KERNELS) for f in KERNELS[:i]]       # (kernel, inherited feature): 21
ALL = dict(K.OPTION, FR_STREAM_BUS="1", FR_STREAM_INPUTS="1", FR_STREAM_BANKS="1", FR_STREAM_LOOPS="1", FR_STREAM_GENERAL="1", FR_STREAM_DYN="1")
IDLE = dict(L.IDLE)
FINITE_SHARE = 0.95
TAIL = [(5003, 300), (69, 200)]
SECOND_STREAM = [(269, 150)]
RING_FRAMES = 32768                                                       # a feedback plan's rings
# A loop of one frame turns everything behind a poisoned time value NaN until the next seek, so the segments' last blocks
# together bound what a sequence can lose.  The layout fixes two of them (the fourth block of 150 frames is 21 long, the fifth of
# 200 is 34); the seed of the time rows, one per layout (by the first segment's length), is the first whose four last blocks
# together stay below POISONED_SHARE of the sequence's frames: whatever the patch, FINITE_SHARE holds for the time rows' part.
POISONED_SHARE = 0.045
TIME_SEED = {700: 2, 1300: 0}


def features_of(s):
    """The features that fr_plan_json["stream"] shows."""
    shown = {"prog": sum(s["programs_per_voice"]) > 0, "bus": s["bus_programs"] > 0, "in": len(s["input_slots"]) > 1,
             "banks": len(s.get("banks", ())) > 1, "loops": any(s.get("loop_programs", ())), "general": len(s.get("general_voices", ())) > 0,
             "dyn": s.get("dyn_reads", 0) + s.get("dyn_steps", 0) > 0}
    return frozenset(f for f, on in shown.items() if on)


# ---- the two patches that no case module has -----------------------------------------------------------------------------------

def dyn_banks_tree(sizes=((1, 256), (2, 128))):
    """Row v = voice v + Delay(voice v, 1 + 30 * lfo) over voices of two sizes: the dyn kernel with several banks."""
    g = synth.GraphArrays()
    v = np.concatenate([D._voices(g, V, P, 0x5EED0B00 + P) for V, P in sizes])
    return D._to_rows(g, g.binop(synth.K_SUM2, v, D._delay(g, v, D._lfo_amount(g), len(v)), len(v)))


def all_features_tree():
    """Voices a = 1 x 256 (balanced) and b = 2 x 100 (schedule voices).  Row 0: x = a + 0.6 * Delay(x, 5); row 1: b0 * In(1) +
    0.25 * Delay(b0, 1 + 30 * lfo); row 2: 0.5 * b0 + 0.25 * b1 (the gains keep the matcher from folding b0 + b1 into one
    voice of 200 leaves: without them there is no bus)."""
    g = synth.GraphArrays()
    f = np.float32
    a = D._voices(g, 1, 256, 0x5EED0B10)
    b = D._voices(g, 2, 100, 0x5EED0B11)
    x = L._loop(g, a, [(5, 0.6)], 1)
    wet = g.binop(synth.K_MUL, D._delay(g, b[:1], D._lfo_amount(g), 1), synth.C(f(0.25)), 1)
    row1 = g.binop(synth.K_SUM2, I._times_input(g, b[:1], 1), wet, 1)
    row2 = g.binop(synth.K_SUM2, g.binop(synth.K_MUL, b[:1], synth.C(f(0.5)), 1), g.binop(synth.K_MUL, b[1:], synth.C(f(0.25)), 1), 1)
    return D._to_rows(g, np.concatenate([x, row1, row2]))


# ---- the table -----------------------------------------------------------------------------------------------------------------

def _case(name, kernel, build, n_rows, options, features=(), n_in=1, semantics="reference", loop=None, oracle_frames=None, delay_rows=(),
          sensitivity=0.90, knob=False):
    """loop: the taps of the patch's feedback loop (None: a feed-forward patch); oracle_frames: None = what the loop's taps cost
    within stream_loop_cases.ORACLE_BUDGET, the whole first segment for a feed-forward patch."""
    first = 700 if loop else 1300
    if oracle_frames is None:
        oracle_frames = L.oracle_frames(loop) if loop else first
    return {"name": name, "kernel": kernel, "build": build, "n_rows": n_rows, "options": options, "features": frozenset(features), "n_in": n_in,
            "semantics": semantics, "feedback": bool(loop), "oracle_frames": min(oracle_frames, first), "delay_rows": list(delay_rows),
            "sensitivity": sensitivity, "knob": knob, "streams": [[(0, first)] + TAIL, SECOND_STREAM], "time_seed": TIME_SEED[first]}


def _of_loops(c, **kw):
    """A case of stream_loop_cases.SERVABLE: its loop's taps from its name's tree (the oracle budget is the module's own)."""
    feats = {"loops"} | ({"prog"} if any(c["per_voice"]) else set()) | ({"bus"} if c["bus"] else set()) | ({"in"} if c["n_in"] > 1 else set())
    feats |= {"banks"} if c["options"] is L.BANKS else set()
    return _case(kw.pop("name", c["name"]), "loops", c["build"], c["n_rows"], c["options"], feats, c["n_in"], loop=(1,), oracle_frames=c["oracle_frames"],
                 delay_rows=range(c["n_rows"]), sensitivity=0.25 if c["name"] == "arith_loop" else 0.90, **kw)


def _of_general(name, feats, **kw):
    c = G.case(name)
    return _case(name, "general", c["build"], c["n_rows"], c["options"], {"general"} | set(feats), c["n_in"], oracle_frames=c["oracle_frames"], **kw)


def _of_dyn(name, feats, **kw):
    c = D.case(name)
    return _case(kw.pop("as_name", name), "dyn", c["build"], c["n_rows"], c["options"], {"dyn"} | set(feats), c["n_in"], oracle_frames=c["oracle_frames"], **kw)


CASES = [
    # plain: one balanced bank straight to the rows; 1 x 1024 is 8 chunks (the chunk tickets)
    _case("plain_2x128", "plain", lambda: synth.additive_tree(2, 128), 2, K.OPTION),
    _case("plain_1x1024", "plain", lambda: synth.additive_tree(1, 1024), 1, K.OPTION),
    # prog: taps of 64, 128 and 192 frames read exactly one block back and further; comb(64) is no loop program
    _case("taps_64_2x128", "prog", lambda: synth.effects_tree(2, 128, envelope=False, taps=3, base_delay=64.0), 2, K.OPTION, {"prog"}, delay_rows=[0, 1]),
    _case("comb_64_2x128", "prog", lambda: K.comb_tree(2, 128, 64), 2, K.OPTION, {"prog"}, loop=(64,), delay_rows=[0, 1]),
    # bus: 3 voices to 2 buses (bus 1 is one voice alone: a program of that voice); a comb behind the bus; rows next to their mix
    _case("mix_3x128_2", "bus", lambda: B.mixdown_tree(3, 128, 2), 2, B.OPTION, {"bus", "prog"}),
    _case("bus_comb_64_2x128", "bus", lambda: B.bus_comb_tree(2, 128, 64), 1, B.OPTION, {"bus"}, loop=(64,), delay_rows=[0]),
    _case("rows_and_bus_3x128", "bus", lambda: B.rows_and_bus_tree(3, 128), 4, B.OPTION, {"bus", "prog"}),
    # in: a gain per voice; seven slots (the doorbell of 8 rows); control rows in a bus program
    _case("gain_2x128", "in", lambda: I.gain_tree(2, 128), 2, I.OPTION, {"in", "prog"}, n_in=3),
    _case("slots_7_2x128", "in", lambda: I.slots_tree(2, 128, 7), 2, I.OPTION, {"in", "prog"}, n_in=7),
    _case("in_bus_3x128", "in", lambda: I.bus_tree(3, 128), 1, I.OPTION, {"in", "bus"}, n_in=5),
    # banks: two sizes to rows; a dry and an enveloped bank; a gated chord on two buses (bus 1 is voice 1 alone)
    _case("rows_256_128", "banks", lambda: M.rows_tree([(1, 256), (2, 128)]), 3, M.OPTION, {"banks"}),
    _case("dry_and_enveloped_128", "banks", lambda: M.dry_and_enveloped_tree(1, 1, 128), 2, M.OPTION, {"banks", "prog"}),
    _case("chord_gated_256_128", "banks", lambda: M.chord_tree(sizes=[(1, 256), (2, 128)], buses=2, gated=True), 2, M.OPTION, {"banks", "bus", "in", "prog"}, n_in=3),
] + [_of_loops(c) for c in L.SERVABLE] + [
    _of_loops(L.case("comb_5_2x128"), name="comb_5_2x128_sparkle", semantics="sparkle"),
    # general: the schedule kernel's own smallest voices, then each inherited feature
    _of_general("additive_2x16", ()),
    _of_general("additive_2x24", ()),
    _of_general("additive_2x100", ()),
    _case("comb_5_2x100", "general", G.case("comb_5_2x100")["build"], 2, G.LOOPS, {"general", "loops", "prog"}, loop=(5,),
          oracle_frames=G.case("comb_5_2x100")["oracle_frames"], delay_rows=[0, 1]),
    _of_general("bus_3x100_2", {"bus", "prog"}),
    _of_general("gain_2x24", {"in", "prog"}),
    _of_general("mixed_banks", {"banks", "prog"}),
    # dyn: amounts of 3..23 frames (reads of the block itself and across its boundary), then each inherited feature
    _of_dyn("chorus_short", {"prog"}),
    _case("beside_loop", "dyn", D.case("beside_loop")["build"], 4, D.LOOPS, {"dyn", "loops", "prog"}, loop=(5,),
          oracle_frames=D.case("beside_loop")["oracle_frames"], delay_rows=[0, 1]),
    _of_dyn("knob", {"in", "prog"}, knob=True),
    _of_dyn("knob", {"in", "prog"}, knob=True, semantics="sparkle", as_name="knob_sparkle"),
    _of_dyn("cross_3", {"bus"}),
    _of_dyn("chorus_2x100", {"general", "prog"}),
    _case("dyn_two_banks", "dyn", dyn_banks_tree, 3, ALL, {"dyn", "banks", "prog"}, oracle_frames=G.ORACLE_LEAF_BUDGET // (512 * 2)),
] + [
    # row 0 is a comb(5) of one voice of 256 partials; rows 1 and 2 cost the oracle 3 + 2 voices of 100 per frame
    _case("all_features" + tag, "dyn", all_features_tree, 3, ALL, set(KERNELS), n_in=2, semantics=sem, loop=(5,),
          oracle_frames=L.oracle_frames((5,), G.ORACLE_LEAF_BUDGET // 256 // 2), delay_rows=[0])
    for tag, sem in (("", "reference"), ("_sparkle", "sparkle"))
]
ALL_FEATURES = "all_features"

# the ring of a feedback plan holds 32768 frames: (name, voices, streams, frames the oracle reaches)
WRAPS = [
    {"name": "wrap_comb_5_1x128", "build": lambda: K.comb_tree(1, 128, 5), "n_rows": 1, "options": L.OPTION, "kernel": "loops",
     "streams": [[(0, 33500)]], "oracle_frames": L.oracle_frames((5,)), "semantics": "reference", "n_in": 1, "knob": False, "time_seed": 0},
    {"name": "wrap_comb_5_2x128_seek", "build": lambda: K.comb_tree(2, 128, 5), "n_rows": 2, "options": L.OPTION, "kernel": "loops",
     "streams": [[(32300, 700)]], "oracle_frames": 0, "semantics": "reference", "n_in": 1, "knob": False, "time_seed": 1},
]


def case(name):
    for c in CASES + WRAPS:
        if c["name"] == name:
            return c
    raise KeyError(name)


def last_blocks(blocks):
    """The numbers of the blocks that end a segment of the stream `blocks`."""
    return {k for k, (idx, T, _) in enumerate(blocks) if k + 1 == len(blocks) or blocks[k + 1][0] != idx + T}


def finite_controls(blocks):
    """The stream's blocks with the control rows' +-inf and NaN kept only in the blocks that end a segment, as finite_block_rows
    keeps the time row's: elsewhere each becomes -2.5, a finite member of stream_input_cases.HOSTILE.  A row that is a voice
    times a control row is NaN wherever the control row is; with blocks_of's rows as they are, such rows are 76 % (seven slots)
    to 94 % (one slot) finite, below FINITE_SHARE.  The zeros, denormals and negative values stay everywhere."""
    last = last_blocks(blocks)
    return [(idx, T, rows if k in last else [rows[0]] + [np.where(np.isfinite(r), r, np.float32(-2.5)).astype(np.float32) for r in rows[1:]])
            for k, (idx, T, rows) in enumerate(blocks)]


def streams_of(c):
    """The case's streams: [[(idx, T, rows)]].  The time rows come from the layout's seed (TIME_SEED), the control rows from a
    generator seeded by the case's name."""
    rng_t, rng = np.random.default_rng(c["time_seed"]), np.random.default_rng(zlib.crc32(c["name"].encode()))
    out = []
    for starts in c["streams"]:
        blocks = finite_controls(L.blocks_of(K.finite_block_rows(rng_t, starts), rng, c["n_in"]))
        out.append(D.knob_blocks(blocks) if c["knob"] else blocks)
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


def poisoned_frames(c):
    """The frames of the blocks that end a segment: the most that poison in the time row can turn NaN."""
    return sum(blocks[k][1] for blocks in streams_of(c) for k in last_blocks(blocks))


def frames_of(c):
    return sum(n for starts in c["streams"] for _, n in starts)


def frames_beyond_oracle(c):
    """The frames of the case's sequence that only the dense reference checks: all but the first segment's leading oracle_frames."""
    return frames_of(c) - c["oracle_frames"]
