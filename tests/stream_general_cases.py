"""Patches for block streaming of voices of any partial count (FR_STREAM_GENERAL on top of FR_STREAM_PROGRAMS), shared by the
simulator tests of the serving rule (tests/test_stream_general_sim.py) and the GPU tests of the resident kernel
(tests/test_hip_stream_general.py).  Graph recipes and plain data: importable without a GPU.

A SCHEDULE voice is a voice the kernel renders item by item in one workgroup: a general voice (any Sum2 tree; the matcher cuts
it into complete sub-trees of 2^k leaves, k <= 11, plus a merge schedule) or a balanced voice of 32 or 64 partials (one item).
The sizes are the smallest that reach each branch of the kernel's item loop (synth.sum_tree pairs neighbours level by level
and carries an odd one up, so P partials fall into the items of P's binary digits):
  2 x 16     one item of two groups (2 waves)                 2 x 24    16 + 8: a two-wave item and a wave-0 group
  2 x 100    64 + (32 + 4): 8 waves, 4 waves, a padded group   2 x 129   128 + 1: a 16-wave item and a one-leaf item
  2 x 300    256 + 32 + 8 + 4                                 2 x 1000  512 + 256 + 128 + 64 + 32 + 8
  1 x 3000   2048 + 512 + 256 + 128 + 32 + 16 + 8: the largest item kind, 16 groups per wave
  balanced 2 x 32 and 2 x 64: one-item schedules the engine synthesises.
Shapes: a left chain of 20 leaves (nothing but merges of single leaves above a pair), and a root that adds a balanced 128-leaf
sub-tree to a 3-leaf one, both ways round: the operand order of the merge.
Expectations come from the graph: `general_voices` is the leaf count of every voice; a plan of schedule voices alone has one
workgroup per voice; programs are dealt as for any other voice (stream_loop_cases, stream_bus_cases, stream_input_cases)."""
import numpy as np

import stream_banks_cases as M
import stream_bus_cases as B
import stream_cases as K
import stream_input_cases as I
import stream_loop_cases as L
from libfriendship_amd import synth
from stream_loop_cases import IDLE, blocks_of, fill_compare, stream_all   # noqa: F401  (the tests take them from here)
from stream_cases import block_rows, short_blocks, silence_voice         # noqa: F401

NEW_KERNEL = "bank_stream_general_kernel"
NEW_KEYS = ("general_voices", "general_max_leaves")
PROGRAMS = dict(K.OPTION)                                       # FR_STREAM_PROGRAMS alone
OPTION = dict(PROGRAMS, FR_STREAM_GENERAL="1")
LOOPS = dict(OPTION, FR_STREAM_LOOPS="1")
BUS = dict(OPTION, FR_STREAM_BUS="1")
INPUTS = dict(OPTION, FR_STREAM_INPUTS="1")
BANKS = dict(OPTION, FR_STREAM_BANKS="1")
MAX_LEAVES = 32768                                              # csrc/streamplan.hpp STREAM_GENERAL_MAX_LEAVES
OLD_GENERAL = "block streaming needs balanced template voices (these are general, compiled or track voices)"
OLD_SMALL = "block streaming needs voices of at least 128 partials (16 waves x one group of 8)"
# The oracle evaluates every leaf of every frame in a tree walk: the comparison with it covers the leading frames whose leaf
# evaluations stay within this many (about two seconds); the comparison with fr_fill_buffer covers every sample.
ORACLE_LEAF_BUDGET = 3000000


def _leaves(g, V, P, seed=0x5EED0900):
    p = synth.voice_params(V, P, seed, True, wrap=24)
    return synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P)


def _to_rows(g, roots):
    roots = np.asarray(roots, dtype=np.uint32)
    g.edge(roots, 0, 0, np.arange(len(roots), dtype=np.uint32))
    return g.finish(len(roots))


def chain_tree(V, P):
    """((((l0 + l1) + l2) + l3) ... + l(P-1)): a left chain."""
    g = synth.GraphArrays()
    lv = _leaves(g, V, P)
    acc = lv[:, 0]
    for k in range(1, P):
        acc = g.binop(synth.K_SUM2, acc, lv[:, k], V)
    return _to_rows(g, acc)


def lopsided_tree(V, mirror):
    """balanced(128 leaves) + ((a + b) + c), or with `mirror` the operands of the root the other way round."""
    g = synth.GraphArrays()
    lv = _leaves(g, V, 131)
    big = synth.sum_tree(g, lv[:, :128])
    small = g.binop(synth.K_SUM2, g.binop(synth.K_SUM2, lv[:, 128], lv[:, 129], V), lv[:, 130], V)
    return _to_rows(g, g.binop(synth.K_SUM2, small, big, V) if mirror else g.binop(synth.K_SUM2, big, small, V))


def mixed_tree():
    """Row 0: a balanced voice of 256 partials; rows 1, 2: voices of 100 partials x the ADSR (they go to rings, a program each);
    rows 3, 4: balanced voices of 64 partials."""
    g = synth.GraphArrays()
    big = synth.sum_tree(g, _leaves(g, 1, 256, 0x5EED0910))
    mid = synth.sum_tree(g, _leaves(g, 2, 100, 0x5EED0911))
    env = synth.adsr_envelope(g)
    mid = g.binop(synth.K_MUL, np.broadcast_to(env, mid.shape), mid, 2)
    low = synth.sum_tree(g, _leaves(g, 2, 64, 0x5EED0912))
    return _to_rows(g, np.concatenate([big, mid, low]))


def _case(name, build, n_rows, options, leaves, per_voice=None, bus=0, n_in=1, loop_delays=None, wgs=None, strides=()):
    """leaves: general_voices (sorted where the plan's bank order decides); per_voice: programs_per_voice, sorted;
    wgs: the launch's workgroups (None: one per voice); loop_delays: the taps of a loop every voice sits in (the oracle's cost)."""
    V = len(leaves)
    frames = ORACLE_LEAF_BUDGET // sum(leaves)
    if loop_delays:                                              # voice evaluations per voice, as stream_loop_cases counts them
        frames = L.oracle_frames(loop_delays, ORACLE_LEAF_BUDGET // sum(leaves))
    return {"name": name, "build": build, "n_rows": n_rows, "options": options, "leaves": list(leaves), "per_voice": sorted(per_voice or [0] * V),
            "bus": bus, "n_in": n_in, "oracle_frames": frames, "wgs": wgs, "strides": list(strides)}


SERVABLE = [_case(f"additive_{V}x{P}", (lambda V=V, P=P: synth.additive_tree(V, P)), V, OPTION, [P] * V)
            for V, P in ((2, 16), (2, 24), (2, 100), (2, 129), (2, 300), (2, 1000), (1, 3000), (2, 32), (2, 64))] + [
    _case("left_chain_20", lambda: chain_tree(2, 20), 2, OPTION, [20, 20]),
    _case("128_plus_3", lambda: lopsided_tree(2, False), 2, OPTION, [131, 131]),
    _case("3_plus_128", lambda: lopsided_tree(2, True), 2, OPTION, [131, 131]),
    _case("comb_5_2x100", lambda: K.comb_tree(2, 100, 5), 2, LOOPS, [100, 100], [1, 1], loop_delays=(5,), strides=[5, 5]),
    # 3 voices to 2 buses: bus 0 = two voices (a bus program), bus 1 = one voice alone (a program of that voice)
    _case("bus_3x100_2", lambda: B.mixdown_tree(3, 100, 2), 2, BUS, [100] * 3, [0, 0, 1], bus=1),
    _case("gain_2x24", lambda: I.gain_tree(2, 24, shared=True), 2, INPUTS, [24, 24], [1, 1], n_in=2),
    # 256 balanced: 2 chunks of 128 (the chunked banks share the workgroups the schedule voices leave)
    _case("mixed_banks", mixed_tree, 5, BANKS, [64, 64, 100, 100], [0, 0, 0, 1, 1], wgs=2 + 4),
]
for _c in SERVABLE:
    if _c["name"] == "mixed_banks":
        _c["voices"] = 5
        _c["banks"] = [(1, 256, False, False), (2, 64, False, True), (2, 100, True, True)]   # (voices, partials, to_ring, general), sorted

# (name, builder, output rows, options, fragments of the reason with FR_STREAM_GENERAL on)
REFUSED = [
    ("too_many_leaves", lambda: synth.additive_tree(1, 40000), 1, OPTION, ("a voice of 40000 leaves", f"at most {MAX_LEAVES} leaves")),
    ("more_voices_than_cus", lambda: synth.additive_tree(257, 16), 257, OPTION, ("one voice per CU",)),
    # triangle voices are compiled voices where there is a run-time compiler ("compiled or track voices": the text is checked on
    # a hand-built bank in tests/cpp/streamgeneral_tests.cpp); the simulator has none, plans them as programs and finds no bank
    ("compiled_voices", lambda: _triangle_tree(2, 128), 2, OPTION, ("block streaming needs a plan with one voice bank (this one: 0 bank launches)",)),
]


def _triangle_tree(V, P):
    g = synth.GraphArrays()
    p = synth.voice_params(V, P, 0x5EED0920, True, wrap=24)
    return _to_rows(g, synth.sum_tree(g, synth.triangle_leaves(g, p["w"], p["amp"]).reshape(V, P)))


def case(name):
    for c in SERVABLE:
        if c["name"] == name:
            return c
    raise KeyError(name)


def check_stream_object(s, c):
    """fr_plan_json["stream"] of a servable case against the graph's expectations."""
    assert s["servable"] is True and s["reason"] == "", s
    assert s["kernel"] == NEW_KERNEL, s
    assert s["general_max_leaves"] == MAX_LEAVES and sorted(s["general_voices"]) == sorted(c["leaves"]), s
    assert s["voices"] == c.get("voices", len(c["leaves"])), s
    assert sorted(s["programs_per_voice"]) == c["per_voice"] and s["bus_programs"] == c["bus"], s
    assert len(s["input_slots"]) == c["n_in"], s
    if c["wgs"] is None:                                         # schedule voices alone: one workgroup per voice, no chunks
        assert s["chunks"] == 1 and s["voices"] == len(c["leaves"]), s
    if "banks" in s:                                             # (FR_STREAM_BANKS)
        got = [(b["voices"], b["partials"], b["to_ring"], b["general"]) for b in s["banks"]]
        assert sorted(got) == c["banks"], s
        assert all(b["chunks"] == 1 for b in s["banks"] if b["general"]), s
        # global voice order: banks in plan order, a schedule bank's voices one after the other
        assert s["general_voices"] == [p for v, p, _, gen in got if gen for _ in range(v)], s
        chunked = [(v, p) for v, p, _, gen in got if not gen]
        chunks = M.deal(chunked, s["max_workgroups"] - sum(v for v, _, _, gen in got if gen))
        assert [b["chunks"] for b in s["banks"] if not b["general"]] == chunks, (s, chunks)
        assert s["workgroups"] == sum(v * ch for (v, _), ch in zip(chunked, chunks)) + sum(v for v, _, _, gen in got if gen), s
        if s["max_workgroups"] == 256:
            assert s["workgroups"] == c["wgs"], s
    if c["strides"]:
        assert sorted(l for l in s["loop_programs"] if l) == c["strides"], s
