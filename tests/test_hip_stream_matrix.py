"""The resident streaming kernels against a dense f32 reference, every sample: the matrix of tests/stream_matrix.py on the GPU.
Every case -- each kernel at its smallest plan, every (kernel, inherited feature) pair of the cascade, the patch with all seven
features, sparkle semantics on three of them, and two feedback plans whose 32768-frame rings wrap -- goes block by block through
fr_stream_block_rows of ONE renderer: a stream from frame 0, a seek forward to frame 5003, a seek back to 69, then fr_stream_end,
fr_stream_begin and a second stream from 269.  After the first block of each stream fr_plan_json names the kernel that runs.
Every streamed sample must equal tests/stream_reference.py's expected_blocks bit for bit, NaN equal to NaN, +0 unequal to -0.

The reference is numpy: it shares nothing with the engine -- not delay_frames, the planner, the rings' capacity or the seek's
warm-up call, which the older tests' comparison of fr_stream_block_rows with fr_fill_buffer has on both sides.
tests/test_stream_matrix.py proves it on the CPU against the simulator's fr_fill_buffer (every block) and the C++ oracle (as far
as its budget reaches), and proves that the inputs keep every row at least 95 % finite; each case here asserts how many of its
frames lie beyond the oracle's reach.

The reference is rendered before the stream opens (nothing slow happens between two blocks of a resident launch) and compared
after it is closed.  A block that is not answered ends the stream within the engine's own bounds (250 ms per block,
FR_STREAM_IDLE_MS for the launch)."""
import pytest

import stream_matrix as X
import stream_reference as SR
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in list(X.ALL) + ["FR_LOOP_TILES", "FR_STREAM_IDLE_MS", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"]:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def stream_case(hip_lib, c, tree, streams):
    """The case's streams through fr_stream_block_rows of one renderer; returns the blocks' results per stream."""
    got = []
    with Renderer(hip_lib, semantics=c["semantics"], options=dict(c["options"], **X.IDLE)) as r:
        synth.install(r, tree)
        for s, blocks in enumerate(streams):
            r.stream_begin(c["n_rows"])
            out = []
            for k, (idx, T, rows) in enumerate(blocks):
                out.append(r.stream_block_rows(idx, rows, n_times=T))
                if k == 0:
                    st = r.plan()["stream"]
                    assert st["servable"] and st["kernel"] == X.KERNEL_NAME[c["kernel"]], (c["name"], s, st)
            r.stream_end()
            got.append(out)
    return got


def compare(c, streams, got, expected):
    """Every sample of every block; returns the frames compared."""
    n = 0
    for s, (blocks, out, exp) in enumerate(zip(streams, got, expected)):
        assert len(out) == len(blocks)
        for k, ((idx, T, _), a, e) in enumerate(zip(blocks, out, exp)):
            assert not SR.first_diff(a, e, f"{c['name']} ({X.KERNEL_NAME[c['kernel']]}) stream {s} block {k} at frame {idx} (T={T}), streamed against the reference")
            n += T
    return n


@pytest.mark.parametrize("name", [c["name"] for c in X.CASES])
def test_every_streamed_sample_equals_the_reference(hip_lib, name):
    c = X.case(name)
    tree, streams, expected = X.reference_of(name)
    got = stream_case(hip_lib, c, tree, streams)
    n = compare(c, streams, got, expected)
    assert n == X.frames_of(c)
    # what only the dense reference checks: the frames past the oracle's budget in the first segment, both seeks, the second stream
    assert n - c["oracle_frames"] == X.frames_beyond_oracle(c) >= 650, (n, c["oracle_frames"])
    print(f"{name}: {n} frames compared, {n - c['oracle_frames']} beyond the oracle's {c['oracle_frames']}")


@pytest.mark.parametrize("name", [c["name"] for c in X.WRAPS])
def test_the_rings_of_a_feedback_plan_wrap(hip_lib, name):
    """comb(5) past the 32768 frames its rings hold -- 33 500 consecutive frames of one voice, and two voices that the ordinary
    path warms up to frame 32 300 --, with at least 95 % of the samples beyond frame 32768 finite."""
    c = X.case(name)
    tree, streams, expected = X.reference_of(name)
    got = stream_case(hip_lib, c, tree, streams)
    n = compare(c, streams, got, expected)
    assert n == X.frames_of(c) and streams[0][-1][0] + streams[0][-1][1] > X.RING_FRAMES
    share = SR.finite_share(got[0], X.RING_FRAMES, [idx for idx, _, _ in streams[0]])
    assert (share >= X.FINITE_SHARE).all(), share
    print(f"{name}: {n} frames compared, {n - c['oracle_frames']} beyond the oracle's {c['oracle_frames']}; finite beyond frame {X.RING_FRAMES}: {share}")
