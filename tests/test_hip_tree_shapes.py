"""The schedule kernels over the shape matrix of tests/tree_shapes.py, on the MI355X: every output sample against the dense f32
reference in each tree's own association (tree_shapes.render_shapes), bit for bit, NaN equal to NaN and +0 unequal to -0.
tests/test_tree_shapes.py pins that reference to the oracle, to a node-by-node restatement and to the simulator on the CPU, and
proves what the table covers.

gbank_kernel and gbank_multi_kernel go through fill_buffer_device as in tests/test_hip_bank_matrix.py: a ramp at 2^20 + 37 of T
frames (no multiple of 64), a hostile row of the same length -- that test's two hostile waves plus three frames of t = +0.0 in one
tile, where every leaf is a zero with its amplitude's sign (the zero-sign repair of single frames, both outcomes) -- and a call of
another length with six such frames in one tile (the zero-sign pass over a whole tile, both outcomes).  Every call asserts the
kernel variant from fr_plan_json's "bank_launches"; the oracle is sought at that test's seek frames.
  gbank_kernel         the whole table in one graph (FR_BANK_MULTI=0): every shape regular and silent, eight shapes in every
                       variant; the voices of 4096 leaves and more as a case of their own with fewer frames
  gbank_multi_kernel   the shapes of at most 128 leaves repeated to 262 voices (one voice per wave), and the shapes of 16 to 32
                       leaves repeated to 1101 voices: two voices of different shape and depth in a row on one wave's stack, the last
                       wave with one voice, the last workgroup with a wave that has none
  bank_stream_general_kernel   two patches of at most 32 voices through fr_stream_block_rows in tests/stream_matrix.py's layout
                       (a stream from frame 0, a seek forward, a seek back, a second stream), every sample of every block"""
import time

import numpy as np
import pytest

import bank_reference
import stream_general_cases as G
import stream_matrix as X
import stream_reference as SR
import test_hip_bank_matrix as BM
import tree_shapes as TS
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in list(X.ALL) + ["FR_BANK_MULTI", "FR_BANK_SHORT", "FR_BANK_TEMPLATE", "FR_BANK_F", "FR_BANK_LEAF", "FR_STREAM_IDLE_MS", "FR_STAGE_JIT"]:
        monkeypatch.delenv(k, raising=False)


def _cycle(shape_names, V):
    """V voices: the shapes over and over, each pass in the next variant the shape has (the first pass regular)."""
    order = ("regular", "silent_neg", "all_neg", "one_pos_padded", "one_pos_16", "one_pos_big", "mixed", "zero_amp", "silent_pos")
    out = []
    while len(out) < V:
        variant = order[(len(out) // len(shape_names)) % len(order)]
        for n in shape_names:
            out.append((n, variant if TS.has_variant(TS.SHAPES[n], variant) else "regular"))
    return out[:V]


def _table():
    """The shapes below 4096 leaves; a few more voices until the row launch's voice count is even and no multiple of 8 (its
    workgroup count is then a multiple of 8 with 4 tiles and is not with 3)."""
    e = TS.table_entries(TS.names(max_leaves=TS.BIG_LEAVES - 1))
    while sum(TS.served(TS.SHAPES[n]) for n, _ in e) % 8 != 2:
        e.append(("depth_16_mixed", TS.VARIANTS[len(e) % len(TS.VARIANTS)]))
    return e


def _big():
    return [(n, v) for v in ("regular", "silent_neg", "all_neg") for n in TS.names(min_leaves=TS.BIG_LEAVES)]


# name: (entries, options, T, T2, kernel variant, voices_per_wave of the first call, [the first call's workgroups are a multiple of 8, the last call's])
CASES = {
    "gbank_kernel": (_table, {"FR_BANK_MULTI": "0"}, 200, 130, "gbank_kernel", 0, [True, False]),
    "gbank_kernel_4096_and_more": (_big, {"FR_BANK_MULTI": "0"}, 70, 33, "gbank_kernel", 0, [True, False]),
    "gbank_multi_kernel_one_voice_per_wave": (lambda: _cycle(TS.names(max_leaves=128, only_served=True), 262), {}, 961, 1030, "gbank_multi_kernel", 1, [True, False]),
    "gbank_multi_kernel_voices_in_a_row": (lambda: _cycle(TS.names(max_leaves=32, min_leaves=16, only_served=True), 1101), {}, 961, 257, "gbank_multi_kernel", 2, [True, False]),
}


def check_call(name, hip, entry, ref, world, idx, row, what, variant, vpw, xcd):
    shapes, w, amp, exp = world
    V = len(shapes)
    got = entry(V, idx, row)
    launches = hip.plan()["bank_launches"]
    # one launch of the voices that go to their rows; the voices under a program (depth_17's inner chain) are a launch of their own
    assert launches and [b["variant"] for b in launches] == [variant] * len(launches) and len(launches) <= 2, f"{name} {what}: ran {launches}"
    served = sum(TS.served(s) for s in shapes)
    under_programs = sum(len(TS.serving_of(s)[0]) for s in shapes if not TS.served(s))
    assert sorted(b["voices"] for b in launches) == sorted(x for x in (served, under_programs) if x), (name, what, launches)
    b = max(launches, key=lambda x: x["voices"])
    assert b["frames"] == len(row) and not b["publishes_rows"], (name, what, b)
    if vpw is not None:
        assert b["voices_per_wave"] == vpw, (name, what, b)
    if xcd is not None:
        assert (BM.workgroups(b) % 8 == 0) == xcd, (name, what, BM.workgroups(b), b)
    msg = bank_reference.first_diff(got, exp, f"{name} {what} (call at {idx}, {len(row)} frames)")
    assert not msg, msg
    for c in BM.seek_frames(len(row), 1):
        o = ref.fill_buffer(V, idx + c, idx + c + 1, [row[c:c + 1]])
        msg = bank_reference.first_diff(exp[:, c:c + 1], o, f"{name} {what}: dense reference vs oracle at frame {c}")
        assert not msg, msg
    return b


@pytest.mark.parametrize("name", list(CASES))
def test_schedule_kernel_against_dense_reference(hip_lib, oracle_lib, name):
    make, options, T, T2, variant, vpw, xcd = CASES[name]
    t0 = time.time()
    entries = make()
    shapes, w, amp = TS.voices(entries)
    tree = TS.build_graph(shapes, w, amp)
    calls = [("ramp", TS.OFFSET, synth.time_ramp(TS.OFFSET, TS.OFFSET + T)),
             ("hostile row", TS.OFFSET + T, TS.hostile_row(TS.OFFSET + T, T)),
             ("second length", TS.OFFSET + 2 * T, TS.second_row(TS.OFFSET + 2 * T, T2))]
    exps = [TS.render_shapes(shapes, w, amp, row) for _, _, row in calls]
    t1 = time.time()
    with Renderer(hip_lib, options=options) as hip, Renderer(oracle_lib) as ref:
        synth.install(hip, tree)
        synth.install(ref, tree)
        entry = BM.Entry(hip, "device")
        for k, ((what, idx, row), exp) in enumerate(zip(calls, exps)):
            b = check_call(name, hip, entry, ref, (shapes, w, amp, exp), idx, row, what, variant,
                           vpw if k == 0 else None, xcd[0] if k == 0 else xcd[1] if k == 2 else None)
            if k == 0 and vpw == 2:      # the last wave has one voice, the last workgroup a wave with none
                assert len(shapes) % 2 == 1 and -(-len(shapes) // 2) % 4 != 0
        plan = hip.plan()
        assert plan["pull_rows"] == 0
        assert plan["stage_programs"] == sum(TS.serving_of(s)[1] for s in shapes)
    zeros = sum(int((e == 0).sum()) for e in exps)
    print(f"{name}: {len(shapes)} voices of {len(set(n for n, _ in entries))} shapes, {sum(TS.n_leaves(s) for s in shapes)} leaves, "
          f"{sum(e.size for e in exps)} samples compared ({zeros} exact zeros), last launch {b['variant']} x {BM.workgroups(b)} workgroups; "
          f"reference {t1 - t0:.2f} s, device and oracle {time.time() - t1:.2f} s")


@pytest.mark.parametrize("patch", sorted(TS.STREAM_PATCHES))
def test_streamed_shapes_against_dense_reference(hip_lib, patch):
    t0 = time.time()
    entries = TS.STREAM_PATCHES[patch]
    shapes, w, amp = TS.voices(entries)
    tree = TS.build_graph(shapes, w, amp)
    V = len(shapes)
    assert V <= 32
    c = X._case("tree_shapes_" + patch, "general", None, V, G.OPTION, {"general"})
    streams = X.streams_of(c)
    # (no Delay in these patches: a block's samples depend on its own time row alone, whatever the seek before it)
    expected = [[TS.render_shapes(shapes, w, amp, rows[0]) for _, _, rows in blocks] for blocks in streams]
    t1 = time.time()
    got = []
    with Renderer(hip_lib, options=dict(G.OPTION, **X.IDLE)) as r:
        synth.install(r, tree)
        for blocks in streams:
            r.stream_begin(V)
            out = []
            for k, (idx, T, rows) in enumerate(blocks):
                out.append(r.stream_block_rows(idx, rows, n_times=T))
                if k == 0:
                    st = r.plan()["stream"]
                    assert st["servable"] and st["kernel"] == G.NEW_KERNEL, st
                    assert st["general_voices"] == [TS.n_leaves(s) for s in shapes] and not any(st["programs_per_voice"]), st
            r.stream_end()
            got.append(out)
    n = 0
    for s, (blocks, out, exp) in enumerate(zip(streams, got, expected)):
        assert len(out) == len(blocks)
        for k, ((idx, T, _), a, e) in enumerate(zip(blocks, out, exp)):
            msg = SR.first_diff(a, e, f"{patch} stream {s} block {k} at frame {idx} (T={T}), streamed against the reference")
            assert not msg, msg + f" ({entries[int(msg.split('row ')[1].split(' ')[0])]})"
            n += T
    assert n == X.frames_of(c) == 1950
    silent = [v for v, (_, variant) in enumerate(entries) if variant in TS.SILENT]
    assert silent and all(not np.nan_to_num(a[v], nan=0.0, posinf=0.0, neginf=0.0).any() for out in got for a in out for v in silent)
    print(f"{patch}: {V} voices, {sum(TS.n_leaves(s) for s in shapes)} leaves, {n} frames in {sum(len(b) for b in streams)} blocks compared; "
          f"reference {t1 - t0:.2f} s, streaming {time.time() - t1:.2f} s")
