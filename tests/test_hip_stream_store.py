"""FR_STREAM_STORE on the GPU: a stream that stores what it is fed and survives edits (bank_stream_store_kernel,
bank_stream_store_fx_kernel; csrc/streamstore.hpp).  Every sequence of tests/stream_store_cases.py -- fr_fill_buffer then a stream,
a stream, an edit and a stream, a stream then fr_fill_buffer, seeks inside a stream, the store's row rules across a boundary -- goes
through ONE renderer with the option on.  Every sample and status must equal, bit for bit (NaN equal to NaN, +0 unequal to -0),
  (a) the same calls and edits through fr_fill_buffer only, on a second HIP renderer with no stream option,
  (b) the C++ oracle, over every step of the sequence that lies before its first seek (the first 300 frames and every boundary).
`store.continued` is asserted after the first block of each continuing stream.  Two long stretches stream past the first slide of
a bounded history's buffer and past the first doubling of an unbounded one; the twin covers them in 4 800-frame calls, the last 8
blocks -- which straddle the relaunch and read back over it -- and an fr_fill_buffer call on the same renderer after the stream are
compared, and the relaunch is counted at its block.  A block that feeds a slot more relaunches too; one that would make nine
streamed slots is refused and leaves no trace.  With the option off the first block after a boundary is the SEEK it has
always been and fr_plan_json has no "store".

tests/test_stream_store_sim.py has proven on the oracle that every expected row is mostly finite and that, at every boundary, a
seek differs from continuing in the first block after it.  One streaming renderer at a time; the twin renders after the stream is
closed.  A block that is not answered ends the stream within the engine's own bounds."""
import numpy as np
import pytest

import stream_reference as SR
import stream_store_cases as S
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INPUT_HISTORY, FR_ERR_UNSUPPORTED, FR_OK, Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN",
              "FR_STREAM_HISTORY", "FR_STREAM_EFFECTS", "FR_STREAM_STORE", "FR_LOOP_TILES", "FR_STREAM_IDLE_MS", "FR_RING_KEEP", "FR_TRACK_HISTORY",
              "FR_DELAY_OBSERVED", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def compare(what, steps, got, exp, upto=None):
    at = S.rendered_steps(steps)
    n = 0
    for k, ((st, a), (st_e, e)) in enumerate(zip(got, exp)):
        if upto is not None and at[k] >= upto:
            break
        s = steps[at[k]]
        where = f"{what}: step {at[k]} ({s[0]} at frame {s[1]}, T={s[2]}, {[len(r) for r in s[3]]} values)"
        assert st == st_e, f"{where}: status {st}, expected {st_e}"
        if st == FR_OK:
            assert not SR.first_diff(a, e, where)
            n += s[2]
    return n


def stream_sequence(hip_lib, p, steps, bounds, options, keep=False):
    """The sequence as written through one renderer with the option on; store.continued is read after every boundary's block."""
    extra = {"FR_RING_KEEP": "1"} if keep else {}
    got, continued = [], {}
    with Renderer(hip_lib, options=dict(options, **S.STORE, **S.IDLE, **extra)) as r:
        p.install(r)
        n_rows = p.n_rows
        for k, s in enumerate(steps):
            res = S.run(r, p, [s], n_rows=n_rows)
            if s[0] == "edit":
                n_rows = getattr(p, "rows_after", {}).get(s[1], n_rows)
            got += res
            if k in bounds and s[0] == "block":
                st = r.plan()["stream"]
                continued[k] = st["store"]["continued"]
                assert st["kernel"] == (S.NEW_FX_KERNEL if p.voiceless else S.NEW_KERNEL) and st["store"]["on"] is True, st
    return got, continued


# (FR_RING_KEEP concerns the first call after a re-plan and the ring table's end: the sequences with an edit or a fill before a stream)
RUNS = [(s, False) for s in S.SEQUENCES] + [(s, True) for s in S.SEQUENCES if s[0] in ("stream_edit_stream", "fill_then_stream")]


@pytest.mark.parametrize("seq,keep", RUNS, ids=[S.sequence_id(s) + ("-ring_keep" if k else "") for s, k in RUNS])
def test_every_sample_and_status(hip_lib, oracle_lib, seq, keep):
    p, steps, bounds, options = S.build(seq)
    got, continued = stream_sequence(hip_lib, p, steps, bounds, options, keep)
    with Renderer(hip_lib, options={"FR_RING_KEEP": "1"} if keep else None) as f:                      # (a)
        p2 = S.build(seq)[0]
        p2.install(f)
        twin = S.run(f, p2, steps, streamed=False)
    assert len(got) == len(twin) == len(S.rendered_steps(steps))
    n = compare(S.sequence_id(seq) + ", streamed against fr_fill_buffer", steps, got, twin)
    assert all(continued[k] is True for k in bounds if steps[k][0] == "block") and len(continued) == sum(steps[k][0] == "block" for k in bounds)
    first_seek = next((k for k, s in enumerate(steps) if s[0] in ("fill", "block") and s[1] > 2000), None)
    with Renderer(oracle_lib) as o:                                                                     # (b)
        p3 = S.build(seq)[0]
        p3.install(o)
        oracle = S.run(o, p3, steps[:first_seek], streamed=False)
    m = compare(S.sequence_id(seq) + ", streamed against the oracle", steps, got, oracle, upto=first_seek)
    assert m >= 295 and all(k < (first_seek or len(steps)) for k in bounds)
    if seq[0] == "row_rules":
        assert [st for st, _ in got][-2:] == [FR_OK, FR_ERR_INPUT_HISTORY]
    print(f"{S.sequence_id(seq)}: {n} frames compared with fr_fill_buffer, {m} with the oracle")


@pytest.mark.parametrize("name", ["tap_100", "comb_441", "echo_in1"])
def test_with_the_option_off_the_first_block_is_a_seek(hip_lib, name):
    """Today's behaviour, pinned: fr_fill_buffer of 150 frames, then a stream at 150 WITHOUT the option -- the stream's blocks equal
    the twin that seeks at 150, differ from the twin that continues, and fr_plan_json has no "store"."""
    p = S.PATCHES[name]()
    steps, bounds = S.seq_fill_then_stream(p)
    with Renderer(hip_lib, options=dict(p.options, **S.IDLE)) as r:
        p.install(r)
        (b,) = bounds
        got = S.run(r, p, steps[:b + 1])
        st = r.plan()["stream"]
        assert "store" not in st and st["kernel"] not in (S.NEW_KERNEL, S.NEW_FX_KERNEL), st
        got += S.run(r, p, steps[b + 1:])
    with Renderer(hip_lib) as f:
        p.install(f)
        seeking = S.run(f, p, steps, streamed=False, seek_at=bounds)
    with Renderer(hip_lib) as f:
        p.install(f)
        continuing = S.run(f, p, steps, streamed=False)
    compare(f"{name}, option off, streamed against the seeking twin", steps, got, seeking)
    k = S.rendered_steps(steps).index(b)
    assert SR.first_diff(got[k][1], continuing[k][1], "the first block after the boundary")


def _long(hip_lib, frames, history_frames, relaunch_block):
    """The stream over [0, frames) in full blocks; the launch is relaunched exactly with block `relaunch_block`, which lies among the
    last 8.  Those 8 blocks -- the ones behind the relaunch read the stream's history 250 frames back, into frames streamed before
    it -- and an fr_fill_buffer call on the SAME renderer after the stream, which reads the store 250 frames back over that frame,
    equal the twin that covered the stretch in 4 800-frame calls."""
    p = S.deep_control_patch()
    blocks, first_compared = S.long_stretch(frames)
    assert first_compared < relaunch_block < len(blocks) - 1 and frames - 250 < relaunch_block * 64 < frames
    control = np.random.default_rng(frames).uniform(0.5, 1.5, size=frames + 64).astype(np.float32)
    rows = lambda idx, T: [synth.time_ramp(idx, idx + T), control[idx:idx + T]]
    got, relaunches = [], {}
    with Renderer(hip_lib, history_frames=history_frames, options=dict(p.options, **S.STORE, **S.IDLE)) as r:
        p.install(r)
        r.stream_begin(p.n_rows)
        for k, (idx, T) in enumerate(blocks):
            a = r.stream_block_rows(idx, rows(idx, T), n_times=T)
            if k >= first_compared:
                got.append(a)
            if k in (relaunch_block - 1, relaunch_block):
                relaunches[k] = r.plan()["stream"]["store"]["relaunches"]
        store = r.plan()["stream"]["store"]
        r.stream_end()
        after = r.fill_buffer(p.n_rows, frames, frames + 64, rows(frames, 64))
    with Renderer(hip_lib, history_frames=history_frames) as f:
        p.install(f)
        start = blocks[first_compared][0]
        for idx in range(0, start, S.LONG_CALL):
            T = min(S.LONG_CALL, start - idx)
            f.fill_buffer(p.n_rows, idx, idx + T, rows(idx, T))
        for (idx, T), a in zip(blocks[first_compared:], got):
            assert not SR.first_diff(a, f.fill_buffer(p.n_rows, idx, idx + T, rows(idx, T)), f"block at frame {idx} of {frames}")
        assert not SR.first_diff(after, f.fill_buffer(p.n_rows, frames, frames + 64, rows(frames, 64)), f"fr_fill_buffer at frame {frames}, after the stream")
    assert len(got) == S.COMPARED and store["continued"] is True   # (a new renderer's head is frame 0)
    assert relaunches == {relaunch_block - 1: 0, relaunch_block: 1} and store["relaunches"] == 1, (relaunches, store)
    assert min(float(np.abs(a).max()) for a in got + [after]) > 0


def test_streamed_past_the_first_slide_of_a_bounded_history(hip_lib):
    _long(hip_lib, S.SLIDE_FRAMES, S.HISTORY_FRAMES, S.SLIDE_BLOCK)


def test_streamed_past_the_first_doubling_of_an_unbounded_history(hip_lib):
    _long(hip_lib, S.DOUBLING_FRAMES, 0, S.DOUBLING_BLOCK)


def _late(hip_lib, oracle_lib, too_many, third=False):
    p = S.late_slots_patch(slot=1 if third else 2)
    steps = S.seq_late_third(p) if third else S.seq_late_slots(p, too_many)
    accepted = [s for s in steps if not (s[0] == "block" and len(s[3]) > 8)]
    got, seen = [], []
    with Renderer(hip_lib, options=dict(p.options, **S.STORE, **S.IDLE)) as r:
        p.install(r)
        for s in steps:
            got += S.run(r, p, [s])
            if s[0] == "block":
                st = r.plan()["stream"]["store"]
                seen.append((st["slots"], st["relaunches"]))
    refused = [x for x, s in zip(got, [s for s in steps if s[0] in ("fill", "block")]) if s[0] == "block" and len(s[3]) > 8]
    got = [x for x, s in zip(got, [s for s in steps if s[0] in ("fill", "block")]) if not (s[0] == "block" and len(s[3]) > 8)]
    for lib, what in ((hip_lib, "fr_fill_buffer"), (oracle_lib, "the oracle")):
        with Renderer(lib) as f:
            p.install(f)
            compare(f"late_slots, streamed against {what}", accepted, got, S.run(f, p, accepted, streamed=False))
    return seen, refused


def test_a_block_that_feeds_a_slot_more_relaunches(hip_lib, oracle_lib):
    """The second block feeds the slots 1 and 2: slot 1 is new to the launch and goes between the rows of the slots 0 and 2, which the
    plan reads.  One relaunch, no seek, and Delay(In(2), 40) goes on reading what was streamed before and after it."""
    seen, _ = _late(hip_lib, oracle_lib, False)
    assert seen[0] == ([0, 2], 0) and all(x == ([0, 1, 2], 1) for x in seen[1:]), seen


def test_a_slot_more_in_the_middle_of_a_stream_refills_the_history(hip_lib, oracle_lib):
    """60 short blocks feed the slots 0 and 1, then a block also feeds slot 2: the history of slot 1, 120 frames of it, is filled
    again from the store, and Delay(In(1), 40) reads it in the blocks behind the relaunch."""
    seen, _ = _late(hip_lib, oracle_lib, False, third=True)
    n = S.LATE_SHORT_BLOCKS
    assert all(x == ([0, 1], 0) for x in seen[:n]) and all(x == ([0, 1, 2], 1) for x in seen[n:]) and len(seen) == n + len(S.LENGTHS), seen


def test_a_block_with_more_slots_than_the_kernel_streams_is_refused_and_leaves_no_trace(hip_lib, oracle_lib):
    seen, refused = _late(hip_lib, oracle_lib, True)
    assert [st for st, _ in refused] == [FR_ERR_UNSUPPORTED]
    assert seen[:2] == [([0, 2], 0), ([0, 2], 0)] and all(x == ([0, 1, 2], 1) for x in seen[2:]), seen
