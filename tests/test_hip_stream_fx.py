"""FR_STREAM_EFFECTS on the GPU: block streaming of patches without a voice (bank_stream_fx_kernel: the resident body with no
bank at all -- a workgroup is one wave that runs a segment of programs, the block's last arriver runs the bus segment).  Every
case of tests/stream_fx_cases.py goes block by block through fr_stream_block_rows of ONE renderer: a stream of 12 blocks -- from
frame 0 with the lengths of stream_cases.FIRST_LENGTHS, a seek forward to frame 5003, a seek back to 69 --, then fr_stream_end,
fr_stream_begin and a second stream from frame 0 again.  Every streamed sample must equal, bit for bit, NaN equal to NaN and +0
unequal to -0,
  (a) fr_fill_buffer of the same calls on a second HIP renderer with no stream option set, statuses included,
  (b) the dense numpy reference (tests/stream_reference.py expected_blocks),
  (c) the C++ oracle over the first segment's 300 frames.
tests/test_stream_fx_sim.py has proven (b) against the simulator and the oracle on the CPU, that every row of it is at least
95 % finite and that a delay one frame off shows.  Three more tests: without the option the patch is refused as before; the
input store's rules (no row, a short row, an empty row after a fed one) through the echo; an edit between two streams.

The shapes: 1 segment, 2 segments, 2 segments and a bus segment, and (rows_260) as many segments as the device has workgroups with
groups that wrap; delays of 1, 3, 5, 64 and 100; a history of 256 frames that wraps within the first 300.  The reference is rendered before the stream opens (nothing slow
happens between two blocks of a resident launch) and compared after it is closed.  Each test has one streaming renderer at a
time.  A block that is not answered ends the stream within the engine's own bounds (250 ms per block, FR_STREAM_IDLE_MS for the
launch)."""
import numpy as np
import pytest

import stream_fx_cases as F
import stream_reference as SR
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_UNSUPPORTED, FR_OK, RenderError, Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN",
              "FR_STREAM_HISTORY", "FR_STREAM_EFFECTS", "FR_LOOP_TILES", "FR_STREAM_IDLE_MS", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED",
              "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def call(fn):
    try:
        return FR_OK, fn()
    except RenderError as e:
        return e.status, None


@pytest.fixture(scope="module")
def device_wgs(hip_lib):
    """The device's workgroups for a resident launch, as the engine counts them: fr_plan_json reports "max_workgroups" with
    FR_STREAM_BANKS, asked once of a renderer of its own (the cases run with their own options)."""
    with Renderer(hip_lib, options=dict(F.OPTION, FR_STREAM_BANKS="1")) as r:
        synth.install(r, F.gain_tree())
        r.fill_buffer(1, 0, 8, [synth.time_ramp(0, 8)])
        n = r.plan()["stream"]["max_workgroups"]
    assert 1 <= n <= F.MAX_WGS
    return n


def stream_case(hip_lib, c, tree, streams, device_wgs):
    """The case's streams through fr_stream_block_rows of one renderer; returns [(status, block)] per stream."""
    got = []
    with Renderer(hip_lib, options=dict(c["options"], **F.IDLE)) as r:
        synth.install(r, tree)
        for s, blocks in enumerate(streams):
            r.stream_begin(c["n_rows"])
            out = []
            for k, (idx, T, rows) in enumerate(blocks):
                out.append(call(lambda: r.stream_block_rows(idx, rows, n_times=T)))
                if k == 0:
                    F.check_stream_object(r.plan()["stream"], c, device_wgs)
            r.stream_end()
            got.append(out)
    return got


def fill_case(lib, c, tree, streams, upto=None):
    """The same calls through fr_fill_buffer of a renderer of `lib` with no option set, a fresh one per stream (its first call is
    a seek, as a stream's first block is); `upto`: the first stream's leading frames only."""
    got = []
    for blocks in streams[:1] if upto is not None else streams:
        out = []
        with Renderer(lib) as f:
            synth.install(f, tree)
            for idx, T, rows in blocks:
                if upto is not None:
                    T = min(T, upto - idx)
                    if T <= 0:
                        break
                out.append(call(lambda: f.fill_buffer(c["n_rows"], idx, idx + T, [r[:T] for r in rows])))
        got.append(out)
    return got


@pytest.mark.parametrize("name", [c["name"] for c in F.SERVABLE])
def test_every_streamed_sample(hip_lib, oracle_lib, device_wgs, name):
    c = F.case(name)
    tree, streams, expected = F.reference_of(name)
    got = stream_case(hip_lib, c, tree, streams, device_wgs)
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
    assert n == F.frames_of(c)
    oracle = fill_case(oracle_lib, c, tree, streams, upto=c["oracle_frames"])[0]                            # (c)
    m = 0
    for k, ((st, a), (st_o, o)) in enumerate(zip(got[0], oracle)):
        assert st_o == FR_OK and not SR.first_diff(a[:, :o.shape[1]], o, f"{name} block {k}, streamed against the oracle")
        m += o.shape[1]
    assert m == c["oracle_frames"] > 0
    print(f"{name}: {n} frames compared with fr_fill_buffer and the reference, {m} with the oracle")


def test_without_the_option_the_patch_is_refused_as_before(hip_lib):
    c = F.case("echo_100")
    with Renderer(hip_lib, options=F.without(dict(c["options"], **F.IDLE), "FR_STREAM_EFFECTS")) as r:
        synth.install(r, c["build"]())
        with pytest.raises(RenderError) as ei:
            r.stream_begin(1)
        assert ei.value.status == FR_ERR_UNSUPPORTED and F.OLD_REASON in str(ei.value), str(ei.value)
        assert r.fill_buffer(1, 0, 32, [synth.time_ramp(0, 32), np.ones(32, np.float32)]).shape == (1, 32)   # the renderer stays usable


def test_the_store_rules_reach_the_echo(hip_lib, device_wgs):
    """Slot 1 gets a full row, a short row, an empty row after a fed one, and at the end no row: what the echo of 100 frames
    makes of them is what fr_fill_buffer makes, and what streamrows.hpp says the slot read (the row, its padding, the slot's last
    value, +0.0)."""
    c = F.case("echo_100")
    tree = c["build"]()
    fed, read = F.store_rule_blocks(np.random.default_rng(100))
    expected = SR.expected_blocks(tree, read)
    got = stream_case(hip_lib, c, tree, [fed], device_wgs)[0]
    filled = fill_case(hip_lib, c, tree, [fed])[0]
    for k, ((idx, T, rows), (st, a), (st_f, b), e) in enumerate(zip(fed, got, filled, expected)):
        what = f"block {k} at frame {idx} ({[len(r) for r in rows]} values)"
        assert st == st_f == FR_OK, (what, st, st_f)
        assert not SR.first_diff(a, b, what + ", streamed against fr_fill_buffer")
        assert not SR.first_diff(a, e, what + ", streamed against the reference of the rows the slot read")
    assert all(np.abs(a).max() > 0.01 for _, a in got[2:])              # the echo goes on when the slot is no longer fed


def test_an_edit_between_two_streams(hip_lib, device_wgs):
    """echo_100 is streamed, the stream ends, the graph becomes comb_5 -- another kernel path: a loop program -- and the second
    stream is correct from frame 0: nothing of the first patch's ring, history or instruction copy is left."""
    a, b = F.case("echo_100"), F.case("comb_5")
    tree_a, streams_a, exp_a = F.reference_of("echo_100")
    tree_b, streams_b, exp_b = F.reference_of("comb_5")
    options = dict(b["options"], **F.IDLE)                                # comb_5's options serve echo_100 too
    with Renderer(hip_lib, options=options) as r:
        synth.install(r, tree_a)
        r.stream_begin(1)
        first = [call(lambda: r.stream_block_rows(idx, rows, n_times=T)) for idx, T, rows in streams_a[1]]
        F.check_stream_object(r.plan()["stream"], a, device_wgs)
        r.stream_end()
        synth.install(r, tree_b)
        r.stream_begin(1)
        second = [call(lambda: r.stream_block_rows(idx, rows, n_times=T)) for idx, T, rows in streams_b[1]]
        F.check_stream_object(r.plan()["stream"], b, device_wgs)
        r.stream_end()
    for what, got, exp in (("before the edit", first, exp_a[1]), ("after the edit", second, exp_b[1])):
        for k, ((st, x), e) in enumerate(zip(got, exp)):
            assert st == FR_OK and not SR.first_diff(x, e, f"block {k} {what}, streamed against the reference")
