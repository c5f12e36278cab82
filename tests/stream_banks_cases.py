"""Patches for block streaming of voices of several banks (FR_STREAM_BANKS on top of FR_STREAM_PROGRAMS), shared by the
simulator tests of the serving rule (tests/test_stream_banks_sim.py) and the GPU tests of the resident kernel
(tests/test_hip_stream_banks.py).

A bank launch is keyed by the voices' partial count and by where they go (a row, or a ring that programs read), so a chord of
notes of several sizes, or dry voices next to enveloped ones, is several banks.  Expectations come from the graph:
  * `banks`: one (voices, partials, to_ring) per distinct size and destination kind;
  * bare voices straight to rows have no programs; a voice times an envelope that goes to its own row is ONE program of that
    voice; voices times gain and envelope summed to B buses are B bus programs and no voice programs; post-bus taps and
    per-size gains from control rows do not add programs (the one-launch form computes a row in one program);
  * the chunks of every bank follow from the rule (`deal`, a restatement of csrc/streamplan.hpp deal_stream_chunks) and the
    workgroup limit the plan reports."""
import numpy as np

import stream_bus_cases as B
import stream_cases as K
import stream_input_cases as I
from libfriendship_amd import synth

PROGRAMS = dict(K.OPTION)                                      # FR_STREAM_PROGRAMS alone
OFF = dict(I.OPTION)                                           # the three older options on, FR_STREAM_BANKS unset: every case is refused
OPTION = dict(OFF, FR_STREAM_BANKS="1")
STREAM_OPTIONS = dict(I.STREAM_OPTIONS, FR_STREAM_BANKS="1")   # (with FR_STREAM_IDLE_MS=1500)
NEW_KERNEL = "bank_stream_banks_kernel"
MAX_BANKS = 8


def old_reason(n_banks):
    return f"block streaming needs a plan with one voice bank (this one: {n_banks} bank launches)"


def _voices(g, V, P, seed):
    p = synth.voice_params(V, P, seed, True, wrap=24)
    return synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P))


def rows_tree(sizes):
    """Bare voices straight to their rows: sizes = [(voices, partials)], rows in that order."""
    g = synth.GraphArrays()
    x = np.concatenate([_voices(g, V, P, 0x5EED0700 + P) for V, P in sizes])
    g.edge(x, 0, 0, np.arange(len(x), dtype=np.uint32))
    return g.finish(len(x))


def dry_and_enveloped_tree(V_dry, V_env, P):
    """Rows 0 .. V_dry-1: bare voices; the next V_env rows: voice x ADSR."""
    g = synth.GraphArrays()
    dry = _voices(g, V_dry, P, 0x5EED0710)
    wet = _voices(g, V_env, P, 0x5EED0711)
    env = synth.adsr_envelope(g)
    wet = g.binop(synth.K_MUL, np.broadcast_to(env, wet.shape), wet, V_env)
    x = np.concatenate([dry, wet])
    g.edge(x, 0, 0, np.arange(len(x), dtype=np.uint32))
    return g.finish(len(x))


CHORD = [(2, 1024), (3, 256), (4, 128)]


def chord_tree(sizes=CHORD, buses=2, post_taps=0, base_delay=100.0, gated=False):
    """A chord: notes of several sizes, every voice x its gain x the ADSR (gated: x In(1 + its size's index) as well), voices
    b::buses summed to bus b, `post_taps` taps per bus."""
    g = synth.GraphArrays()
    env = synth.adsr_envelope(g)
    xs = []
    for k, (V, P) in enumerate(sizes):
        x = _voices(g, V, P, 0x5EED0720 + P)
        if gated:
            x = I._times_input(g, x, 1 + k)
        xs.append(x)
    x = np.concatenate(xs)
    n = len(x)
    x = g.binop(synth.K_MUL, synth.C(B.gains(n)), x, n)
    x = g.binop(synth.K_MUL, np.broadcast_to(env, x.shape), x, n)
    y = B._buses(g, x, buses)
    if post_taps:
        y = synth.delay_chain(g, y, post_taps, base_delay)
    g.edge(y, 0, 0, np.arange(buses, dtype=np.uint32))
    return g.finish(buses)


def general_tree():
    """Two balanced voices of 128 partials and one of 1000 (no power of two: a general voice), to rows."""
    g = synth.GraphArrays()
    x = np.concatenate([_voices(g, 2, 128, 0x5EED0730), _voices(g, 1, 1000, 0x5EED0731)])
    g.edge(x, 0, 0, np.arange(3, dtype=np.uint32))
    return g.finish(3)


NINE = [(1, 128 << k) for k in range(9)]                      # 128 .. 32768 partials

# (name, builder, output rows, options, banks as sorted (voices, partials, to_ring), programs per voice of a bank by to_ring
#  {False: n, True: n}, bus programs, input slots)
SERVABLE = [
    ("rows_two_sizes", lambda: rows_tree([(2, 128), (2, 1024)]), 4, OPTION, [(2, 128, False), (2, 1024, False)], {False: 0, True: 0}, 0, [0]),
    ("dry_and_enveloped", lambda: dry_and_enveloped_tree(2, 2, 256), 4, OPTION, [(2, 256, False), (2, 256, True)], {False: 0, True: 1}, 0, [0]),
    ("chord_bus", lambda: chord_tree(), 2, OPTION, [(2, 1024, True), (3, 256, True), (4, 128, True)], {False: 0, True: 0}, 2, [0]),
    ("chord_bus_taps", lambda: chord_tree(post_taps=1), 2, OPTION, [(2, 1024, True), (3, 256, True), (4, 128, True)], {False: 0, True: 0}, 2, [0]),
    ("chord_gated", lambda: chord_tree(gated=True), 2, OPTION, [(2, 1024, True), (3, 256, True), (4, 128, True)], {False: 0, True: 0}, 2, [0, 1, 2, 3]),
]

# (name, builder, output rows, bank launches of the plan, fragment of the reason with the option on)
REFUSED = [
    ("nine_sizes", lambda: rows_tree(NINE), 9, 9, "at most 8 voice banks in one launch (this plan: 9 bank launches)"),
    ("with_general_voice", general_tree, 3, 2, "block streaming needs balanced template voices (these are general, compiled or track voices)"),
    ("too_many_voices", lambda: rows_tree([(200, 128), (100, 256)]), 300, 2, "block streaming serves at most one voice per CU ("),
]


def case(table, name):
    return K.case(table, name)


def deal(banks, max_wgs):
    """The chunks per voice of every bank: banks = [(voices, partials)] in plan order.  Every bank starts at one chunk per
    voice; then, until none qualifies, the bank with the largest chunk (on a tie the first) among those with chunks above 128
    partials, fewer than 256 chunks per voice and room for twice their workgroups has its chunk halved."""
    size = [P for _, P in banks]
    chunks = [1] * len(banks)
    total = sum(V for V, _ in banks)
    assert total <= max_wgs
    while True:
        ok = [i for i, (V, P) in enumerate(banks) if size[i] > 128 and chunks[i] < 256 and total + V * chunks[i] <= max_wgs]
        if not ok:
            return chunks
        i = max(ok, key=lambda j: (size[j], -j))
        total += banks[i][0] * chunks[i]
        size[i] //= 2
        chunks[i] *= 2


def check_stream_object(s, banks, per_voice, bus, slots):
    """fr_plan_json["stream"] of a servable case against the graph's expectations; returns the reported banks."""
    assert s["servable"] is True and s["reason"] == "", s
    assert s["kernel"] == NEW_KERNEL, s
    got = [(b["voices"], b["partials"], b["to_ring"]) for b in s["banks"]]
    assert sorted(got) == sorted(banks), s
    chunks = deal([(v, p) for v, p, _ in got], s["max_workgroups"])
    assert [b["chunks"] for b in s["banks"]] == chunks, (s, chunks)
    assert s["workgroups"] == sum(v * c for (v, _, _), c in zip(got, chunks)) <= s["max_workgroups"]
    assert s["voices"] == sum(v for v, _, _ in got) and s["chunks"] == max(chunks)
    assert s["programs_per_voice"] == [per_voice[r] for v, _, r in got for _ in range(v)], s
    assert s["bus_programs"] == bus and s["input_slots"] == slots, s
    return got
