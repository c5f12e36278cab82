"""FR_STREAM_HISTORY on the GPU: block streaming of delayed reads of input rows (bank_stream_hist_kernel: the dyn kernel's
composition, a history of the streamed rows that workgroup 0 stores with every block, S_READ_INPUT and S_READ_INPUT_DYN read
from it).  Every case of tests/stream_hist_cases.py goes block by block through fr_stream_block_rows of ONE renderer: a stream
of 12 blocks -- from frame 0 with the lengths of stream_cases.FIRST_LENGTHS, a seek forward to frame 5003, a seek back to 69 --,
then fr_stream_end, fr_stream_begin and a second stream from frame 0 again.  Every streamed sample must equal, bit for bit, NaN
equal to NaN and +0 unequal to -0,
  (a) fr_fill_buffer of the same calls on a second HIP renderer with no stream option set, statuses included,
  (b) the dense numpy reference (tests/stream_reference.py expected_blocks),
  (c) the C++ oracle over the leading frames its budget reaches.
tests/test_stream_hist_sim.py has proven (b) against the simulator and the oracle on the CPU, that every row of it is at least
95 % finite and that a delay one frame off shows.  One more test takes the input store's rules through the history: a slot
that gets no row, a short row, an empty row after a fed one.

The reference is rendered before the stream opens (nothing slow happens between two blocks of a resident launch) and compared
after it is closed.  Each test has one streaming renderer at a time.  A block that is not answered ends the stream within the
engine's own bounds (250 ms per block, FR_STREAM_IDLE_MS for the launch)."""
import numpy as np
import pytest

import stream_hist_cases as H
import stream_reference as SR
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_UNSUPPORTED, FR_OK, RenderError, Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN",
              "FR_STREAM_HISTORY", "FR_LOOP_TILES", "FR_STREAM_IDLE_MS", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def call(fn):
    try:
        return FR_OK, fn()
    except RenderError as e:
        return e.status, None


def stream_case(hip_lib, c, tree, streams):
    """The case's streams through fr_stream_block_rows of one renderer; returns [(status, block)] per stream."""
    got = []
    with Renderer(hip_lib, semantics=c["semantics"], options=dict(c["options"], **H.IDLE)) as r:
        synth.install(r, tree)
        for s, blocks in enumerate(streams):
            r.stream_begin(c["n_rows"])
            out = []
            for k, (idx, T, rows) in enumerate(blocks):
                out.append(call(lambda: r.stream_block_rows(idx, rows, n_times=T)))
                if k == 0:
                    H.check_stream_object(r.plan()["stream"], c)
            r.stream_end()
            got.append(out)
    return got


def fill_case(lib, c, tree, streams, upto=None):
    """The same calls through fr_fill_buffer of a renderer of `lib` with no option set, a fresh one per stream (its first call is
    a seek, as a stream's first block is); `upto`: the first stream's leading frames only."""
    got = []
    for blocks in streams[:1] if upto is not None else streams:
        out = []
        with Renderer(lib, semantics=c["semantics"]) as f:
            synth.install(f, tree)
            for idx, T, rows in blocks:
                if upto is not None:
                    T = min(T, upto - idx)
                    if T <= 0:
                        break
                out.append(call(lambda: f.fill_buffer(c["n_rows"], idx, idx + T, [r[:T] for r in rows])))
        got.append(out)
    return got


@pytest.mark.parametrize("name", [c["name"] for c in H.SERVABLE])
def test_every_streamed_sample(hip_lib, oracle_lib, name):
    c = H.case(name)
    tree, streams, expected = H.reference_of(name)
    got = stream_case(hip_lib, c, tree, streams)
    filled = fill_case(hip_lib, c, tree, streams)
    n = 0
    for s, (blocks, out, fil, exp) in enumerate(zip(streams, got, filled, expected)):
        assert len(out) == len(blocks) == len(fil)
        for k, ((idx, T, _), (st, a), (st_f, b), e) in enumerate(zip(blocks, out, fil, exp)):
            what = f"{name} stream {s} block {k} at frame {idx} (T={T})"
            assert st == st_f == FR_OK, f"{what}: status {st} streamed, {st_f} through fr_fill_buffer"
            assert not SR.first_diff(a, b, what + ", streamed against fr_fill_buffer")                   # (a)
            assert not SR.first_diff(a, e, what + ", streamed against the reference")                    # (b)
            n += T
    assert n == H.frames_of(c)
    oracle = fill_case(oracle_lib, c, tree, streams, upto=c["oracle_frames"])[0]                            # (c)
    m = 0
    for k, ((st, a), (st_o, o)) in enumerate(zip(got[0], oracle)):
        assert st_o == FR_OK and not SR.first_diff(a[:, :o.shape[1]], o, f"{name} block {k}, streamed against the oracle")
        m += o.shape[1]
    assert m == c["oracle_frames"] > 0
    print(f"{name}: {n} frames compared with fr_fill_buffer and the reference, {m} with the oracle")


def test_the_store_rules_reach_the_history(hip_lib):
    """Slot 1 gets a full row, a short row, an empty row after a fed one, and at the end no row: what Delay(In(1), 65) reads back
    65 frames later is what fr_fill_buffer reads, and what streamrows.hpp says the slot read (the row, its padding, the slot's
    last value, +0.0)."""
    c = H.case("gate_65")
    tree = c["build"]()
    fed, read = H.store_rule_blocks(np.random.default_rng(65), 65)
    expected = SR.expected_blocks(tree, read)
    got = stream_case(hip_lib, c, tree, [fed])[0]
    filled = fill_case(hip_lib, c, tree, [fed])[0]
    for k, ((idx, T, rows), (st, a), (st_f, b), e) in enumerate(zip(fed, got, filled, expected)):
        what = f"block {k} at frame {idx} ({[len(r) for r in rows]} values)"
        assert st == st_f == FR_OK, (what, st, st_f)
        assert not SR.first_diff(a, b, what + ", streamed against fr_fill_buffer")
        assert not SR.first_diff(a, e, what + ", streamed against the reference of the rows the slot read")
    assert all(np.abs(a).max() > 0.01 for _, a in got[2:])              # the padding and the zeros arrive 65 frames late, not never


def test_without_the_option_the_patch_is_refused_as_before(hip_lib):
    c = H.case("gate_100")
    with Renderer(hip_lib, options={k: v for k, v in dict(c["options"], **H.IDLE).items() if k != "FR_STREAM_HISTORY"}) as r:
        synth.install(r, c["build"]())
        with pytest.raises(RenderError) as ei:
            r.stream_begin(2)
        assert ei.value.status == FR_ERR_UNSUPPORTED and H.OLD_INPUT in str(ei.value), str(ei.value)
        assert r.fill_buffer(2, 0, 32, [synth.time_ramp(0, 32), np.ones(32, np.float32)]).shape == (2, 32)   # the renderer stays usable
