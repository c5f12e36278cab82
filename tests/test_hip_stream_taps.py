"""FR_STREAM_TAPS on the GPU: block streaming of short and signal delays of computed values -- a plan without a fused form served
in its level form by the resident kernels as they stand (the launch rule's cascade chooses: prog, bus, general, dyn, fx; with
FR_STREAM_HISTORY or FR_STREAM_BANKS next to the option, stream_taps_cases.COMPOSED: hist, banks).  Every case of
tests/stream_taps_cases.py goes block by block through fr_stream_block_rows of ONE renderer: a stream of 12 blocks -- from
frame 0 with the lengths of stream_cases.FIRST_LENGTHS, a seek forward to frame 5003, a seek back to 69 --, then fr_stream_end,
fr_stream_begin and a second stream from frame 0 again.  Every streamed sample must equal, bit for bit, NaN equal to NaN and +0
unequal to -0,
  (a) fr_fill_buffer of the same calls on a second HIP renderer with no stream option set, statuses included,
  (b) the dense numpy reference (tests/stream_reference.py expected_blocks),
  (c) the C++ oracle over the first 300 frames.
tests/test_stream_taps_sim.py has proven (b) against the simulator and the oracle on the CPU, that every row of it is at least
95 % finite, that a constant delay one frame off changes at least 90 % of the samples behind it and a signal amount one frame off at
least half of every row.  Four more tests: without the option the patch is refused as before and the renderer stays usable; both
semantics on env_chorus_2x128; an edit between two streams; with FR_STREAM_STORE, an edit of the chorus depth inside a stream.

What a read below a block relies on is the order inside ONE wave: a program's ring stores are acknowledged (s_waitcnt vmcnt(0))
before the next program's loads, and earlier blocks' frames were acknowledged before their done tag -- env_taps_2x512 has four
chunks per voice, so the voice's finisher changes CU between blocks and both are exercised.  The reference is rendered before the
stream opens (nothing slow happens between two blocks of a resident launch) and compared after it is closed.  Each test has one
streaming renderer at a time.  A block that is not answered ends the stream within the engine's own bounds (250 ms per block,
FR_STREAM_IDLE_MS for the launch)."""
import numpy as np
import pytest

import stream_reference as SR
import stream_taps_cases as T
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_UNSUPPORTED, FR_OK, RenderError, Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN",
              "FR_STREAM_HISTORY", "FR_STREAM_EFFECTS", "FR_STREAM_STORE", "FR_STREAM_TAPS", "FR_LOOP_TILES", "FR_STREAM_IDLE_MS", "FR_RING_KEEP",
              "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def call(fn):
    try:
        return FR_OK, fn()
    except RenderError as e:
        return e.status, None


def stream_case(hip_lib, c, tree, streams, semantics="reference"):
    """The case's streams through fr_stream_block_rows of one renderer; returns [(status, block)] per stream."""
    got = []
    with Renderer(hip_lib, semantics=semantics, options=dict(c["options"], **T.IDLE)) as r:
        synth.install(r, tree)
        for blocks in streams:
            r.stream_begin(c["n_rows"])
            out = []
            for k, (idx, n_t, rows) in enumerate(blocks):
                out.append(call(lambda: r.stream_block_rows(idx, rows, n_times=n_t)))
                if k == 0:
                    T.check_stream_object(r.plan()["stream"], c, launched=True)
            r.stream_end()
            got.append(out)
    return got


def fill_case(lib, c, tree, streams, upto=None, semantics="reference"):
    """The same calls through fr_fill_buffer of a renderer of `lib` with no option set, a fresh one per stream (its first call is
    a seek, as a stream's first block is); `upto`: the first stream's leading frames only."""
    got = []
    for blocks in streams[:1] if upto is not None else streams:
        out = []
        with Renderer(lib, semantics=semantics) as f:
            synth.install(f, tree)
            for idx, n_t, rows in blocks:
                if upto is not None:
                    n_t = min(n_t, upto - idx)
                    if n_t <= 0:
                        break
                out.append(call(lambda: f.fill_buffer(c["n_rows"], idx, idx + n_t, [r[:n_t] for r in rows])))
        got.append(out)
    return got


def compare(name, streams, got, filled, expected):
    n = 0
    for s, (blocks, out, fil, exp) in enumerate(zip(streams, got, filled, expected)):
        assert len(out) == len(blocks) == len(fil)
        for k, ((idx, n_t, _), (st, a), (st_f, b), e) in enumerate(zip(blocks, out, fil, exp)):
            what = f"{name} stream {s} block {k} at frame {idx} (T={n_t})"
            assert st == st_f == FR_OK, f"{what}: status {st} streamed, {st_f} through fr_fill_buffer"
            assert not SR.first_diff(a, b, what + ", streamed against fr_fill_buffer")                   # (a)
            assert not SR.first_diff(a, e, what + ", streamed against the reference")                    # (b)
            n += n_t
    return n


@pytest.mark.parametrize("name", [c["name"] for c in T.ALL])
def test_every_streamed_sample(hip_lib, oracle_lib, name):
    c = T.case(name)
    tree, streams, expected = T.reference_of(name)
    got = stream_case(hip_lib, c, tree, streams)
    filled = fill_case(hip_lib, c, tree, streams)
    n = compare(name, streams, got, filled, expected)
    assert n == T.frames_of(c)
    oracle = fill_case(oracle_lib, c, tree, streams, upto=c["oracle_frames"])[0]                            # (c)
    m = 0
    for k, ((st, a), (st_o, o)) in enumerate(zip(got[0], oracle)):
        assert st_o == FR_OK and not SR.first_diff(a[:, :o.shape[1]], o, f"{name} block {k}, streamed against the oracle")
        m += o.shape[1]
    assert m == c["oracle_frames"] == 300
    print(f"{name}: {n} frames compared with fr_fill_buffer and the reference, {m} with the oracle")


def test_without_the_option_the_patch_is_refused_as_before(hip_lib):
    c = T.case("env_fir_2x128")
    with Renderer(hip_lib, options=T.without(dict(c["options"], **T.IDLE), "FR_STREAM_TAPS")) as r:
        synth.install(r, c["build"]())
        with pytest.raises(RenderError) as ei:
            r.stream_begin(2)
        assert ei.value.status == FR_ERR_UNSUPPORTED and T.NO_FUSED_FORM in str(ei.value), str(ei.value)
        assert r.fill_buffer(2, 0, 32, [synth.time_ramp(0, 32)]).shape == (2, 32)   # the renderer stays usable


@pytest.mark.parametrize("semantics", ["reference", "sparkle"])
def test_both_semantics_of_the_chorus(hip_lib, semantics):
    c = T.case("env_chorus_2x128")
    tree, streams, _ = T.reference_of(c["name"])
    expected = [SR.expected_blocks(tree, blocks, semantics) for blocks in streams]
    got = stream_case(hip_lib, c, tree, streams, semantics)
    filled = fill_case(hip_lib, c, tree, streams, semantics=semantics)
    assert compare(f"{c['name']} ({semantics})", streams, got, filled, expected) == T.frames_of(c)


def test_an_edit_between_two_streams(hip_lib):
    """env_fir is streamed, the stream ends, the graph becomes bus_chorus -- other rings, other programs, another kernel -- and the
    second stream is correct from frame 0: nothing of the first patch's rings or instruction copy is left."""
    a, b = T.case("env_fir_2x128"), T.case("bus_chorus_3x128")
    tree_a, streams_a, exp_a = T.reference_of(a["name"])
    tree_b, streams_b, exp_b = T.reference_of(b["name"])
    options = dict(b["options"], **T.IDLE)                                # bus_chorus's options serve env_fir too
    with Renderer(hip_lib, options=options) as r:
        synth.install(r, tree_a)
        r.stream_begin(a["n_rows"])
        first = [call(lambda: r.stream_block_rows(idx, rows, n_times=n_t)) for idx, n_t, rows in streams_a[1]]
        T.check_stream_object(r.plan()["stream"], a, launched=True)
        r.stream_end()
        synth.install(r, tree_b)
        r.stream_begin(b["n_rows"])
        second = [call(lambda: r.stream_block_rows(idx, rows, n_times=n_t)) for idx, n_t, rows in streams_b[1]]
        T.check_stream_object(r.plan()["stream"], b, launched=True)
        r.stream_end()
    for what, got, exp in (("before the edit", first, exp_a[1]), ("after the edit", second, exp_b[1])):
        for k, ((st, x), e) in enumerate(zip(got, exp)):
            assert st == FR_OK and not SR.first_diff(x, e, f"block {k} {what}, streamed against the reference")


def test_the_tails_survive_an_edit_with_the_store(hip_lib):
    """FR_STREAM_STORE: env_chorus streamed, the chorus depth constant edited, streamed on -- bit for bit the fr_fill_buffer twin
    of the same calls and the same edit, so the frames the chorus reads back across the edit are the ones streamed before it."""
    c = T.case("env_chorus_2x128")
    tree, streams, _ = T.reference_of(c["name"])
    blocks, cut = streams[0][:8], 4                                      # 300 consecutive frames from 0, the edit after 166 of them
    with Renderer(hip_lib) as f:
        synth.install(f, tree)
        twin = [call(lambda: f.fill_buffer(2, idx, idx + n_t, rows)) for idx, n_t, rows in blocks[:cut]]
        T.edit_depth(f, tree)
        twin += [call(lambda: f.fill_buffer(2, idx, idx + n_t, rows)) for idx, n_t, rows in blocks[cut:]]
    seeked = SR.expected_blocks(T.with_depth(tree), blocks[cut:])        # what a stream that seeks at the edit would give
    with Renderer(hip_lib, options=dict(c["options"], FR_STREAM_STORE="1", **T.IDLE)) as r:
        synth.install(r, tree)
        r.stream_begin(2)
        got = [call(lambda: r.stream_block_rows(idx, rows, n_times=n_t)) for idx, n_t, rows in blocks[:cut]]
        s = r.plan()["stream"]
        assert s["servable"] is True and s["kernel"] == "bank_stream_store_kernel" and s["levels"] == 2 and s["dyn_ring_reads"] == 2, s
        r.stream_end()
        T.edit_depth(r, tree)
        r.stream_begin(2)
        got += [call(lambda: r.stream_block_rows(idx, rows, n_times=n_t)) for idx, n_t, rows in blocks[cut:]]
        assert r.plan()["stream"]["store"]["continued"] is True
        r.stream_end()
    for k, ((st, a), (st_f, b)) in enumerate(zip(got, twin)):
        assert st == st_f == FR_OK and not SR.first_diff(a, b, f"block {k}, streamed against the fr_fill_buffer twin")
    assert SR.first_diff(got[cut][1], seeked[0], "the first block after the edit")   # a seek there would have cut the tails: it differs
