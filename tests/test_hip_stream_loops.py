"""FR_STREAM_LOOPS on the GPU: block streaming of feedback loops shorter than a block (bank_stream_loops_kernel: a loop program
runs in the finishing wave in three phases -- frame-only loads into an LDS tile, lanes below the stride walk their residue's
frames on LDS operands, all lanes store).  Blocks go through fr_stream_block_rows from frame 0; then, after the stream is closed
(nothing else renders while a launch is resident), the same blocks go through fr_fill_buffer of a second HIP renderer with no
stream option set -- every sample equal bit for bit, NaN equal to NaN, +0 unequal to -0 -- and the first blocks, up to the
frame stream_loop_cases.oracle_frames gives for the case, through the oracle.  The serving rule: tests/test_stream_loops_sim.py;
the helper and a host model of the three phases: tests/test_stream_loops_host.py.

Each test has one streaming renderer at a time.  A block that is not answered ends the stream within the engine's own bounds
(250 ms per block, FR_STREAM_IDLE_MS for the launch)."""
import numpy as np
import pytest

import stream_loop_cases as L
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_LOOP_TILES", "FR_STREAM_IDLE_MS", "FR_RING_KEEP",
              "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def trees():
    return {}


def tree_of(trees, name):
    if name not in trees:
        trees[name] = L.case(name)["build"]()
    return trees[name]


def loud(got):
    return max(float(np.nanmax(np.abs(np.where(np.isfinite(a), a, 0)))) for a in got)


def run_case(hip_lib, oracle_lib, tree, c, blocks, semantics="reference", oracle=True, streamed=None):
    """Streamed, then every sample against fr_fill_buffer, then the early blocks against the oracle; returns the plan (and the
    streamed blocks in the list `streamed`)."""
    got, plan = L.stream_all(hip_lib, tree, c["n_rows"], blocks, c["options"], semantics)
    if streamed is not None:
        streamed.extend(got)
    L.check_stream_object(plan["stream"], c)
    frames = sum(T for _, T, _ in blocks)
    assert L.fill_compare(hip_lib, tree, c["n_rows"], blocks, got, "through fr_fill_buffer", semantics) == frames
    if oracle:
        assert blocks[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
        assert L.fill_compare(oracle_lib, tree, c["n_rows"], blocks, got, "on the oracle", semantics, upto=c["oracle_frames"]) == min(frames, c["oracle_frames"])
    assert loud(got) > 0.01
    return plan


@pytest.mark.parametrize("name", [c["name"] for c in L.SERVABLE])
def test_every_case_every_sample(hip_lib, oracle_lib, trees, name):
    """About 1500 frames from frame 0 in blocks of random length 1..64, every fifth time row hostile; control rows of every kind."""
    c = L.case(name)
    rng = np.random.default_rng(len(name) * 7919)
    blocks = L.blocks_of(L.block_rows(rng, [(0, 1500)]), rng, c["n_in"])
    run_case(hip_lib, oracle_lib, tree_of(trees, name), c, blocks)


@pytest.mark.parametrize("name", ["comb_1_2x128", "comb_1_2x256", "arith_loop"])
def test_sparkle_semantics(hip_lib, oracle_lib, trees, name):
    c = L.case(name)
    rng = np.random.default_rng(11)
    blocks = L.blocks_of(L.block_rows(rng, [(0, 700)]), rng, c["n_in"])
    run_case(hip_lib, oracle_lib, tree_of(trees, name), c, blocks, semantics="sparkle")


@pytest.mark.parametrize("P", [128, 256])
@pytest.mark.parametrize("d", [1, 63])
def test_short_blocks_with_a_silent_voice(hip_lib, oracle_lib, d, P):
    """A full block, a block of one frame and a block of 37 from frame 0, the last voice silent: exact-zero sums enter the loop;
    in the 64-frame block d = 63 takes its second trip only at frame 63."""
    c = L.case(f"comb_{d}_2x{P}")
    tree = L.silence_voice(c["build"](), 2, P, 1)
    blocks = L.blocks_of(L.short_blocks(idx=0))
    got, plan = L.stream_all(hip_lib, tree, 2, blocks, c["options"])
    L.check_stream_object(plan["stream"], c)
    assert L.fill_compare(hip_lib, tree, 2, blocks, got, "through fr_fill_buffer") == 102
    assert L.fill_compare(oracle_lib, tree, 2, blocks, got, "on the oracle") == 102
    assert [a.shape for a in got] == [(2, 64), (2, 1), (2, 37)]
    assert not any(a[1].any() for a in got) and loud(got) > 0.01


def test_the_rings_wrap(hip_lib, oracle_lib, trees):
    """comb(5) on 2 x 128 for more frames than a feedback plan's rings hold.  The time rows are finite_block_rows': with
    block_rows' a NaN entered the loops in the first hostile block and 2.7 % of the samples were finite, none beyond frame 1878,
    so the frames past the rings' end compared NaN with NaN."""
    c = L.case("comb_5_2x128")
    frames = 33500
    blocks = L.blocks_of(L.finite_block_rows(np.random.default_rng(5), [(0, frames)]))
    got = []
    plan = run_case(hip_lib, oracle_lib, tree_of(trees, c["name"]), c, blocks, streamed=got)
    ring_frames = 32768 if plan["feedback"] else 1024
    assert plan["feedback"] and frames > ring_frames and frames > plan["max_lookback"]
    beyond = np.concatenate([a[:, max(0, ring_frames - idx):] for (idx, _, _), a in zip(blocks, got)], axis=1)
    assert beyond.shape == (2, frames - ring_frames) and np.isfinite(beyond).mean(axis=1).min() >= 0.95, np.isfinite(beyond).mean(axis=1)


@pytest.mark.parametrize("d", [1, 5])
def test_jumps_are_seeks(hip_lib, trees, d):
    """A block that does not continue the previous one retires the launch and replays the loop from frame 0."""
    c = L.case(f"comb_{d}_2x128")
    starts = [(0, 300), (9000, 200), (2500, 200), (40000, 100), (64, 100)]
    blocks = L.blocks_of(L.block_rows(np.random.default_rng(d), starts))
    run_case(hip_lib, None, tree_of(trees, c["name"]), c, blocks, oracle=False)


def test_a_loop_of_a_block_or_more_keeps_its_kernel(hip_lib):
    """comb(64) with the option on: no loop program, the kernel it has always had."""
    tree = L.comb_tree(2, 128, 64)
    blocks = L.blocks_of(L.block_rows(np.random.default_rng(64), [(0, 400)]))
    got, plan = L.stream_all(hip_lib, tree, 2, blocks, L.OPTION)
    s = plan["stream"]
    assert s["servable"] and s["kernel"] == "bank_stream_prog_kernel" and s["loop_programs"] == [0, 0], s
    assert L.fill_compare(hip_lib, tree, 2, blocks, got, "through fr_fill_buffer") == 400


def test_without_the_option_a_short_loop_is_refused_as_before(hip_lib, trees):
    from libfriendship_amd.capi import FR_ERR_UNSUPPORTED, RenderError
    tree = tree_of(trees, "comb_5_2x128")
    with Renderer(hip_lib, options=dict(L.PROGRAMS, **L.IDLE)) as r:
        synth.install(r, tree)
        with pytest.raises(RenderError) as ei:
            r.stream_begin(2)
        assert ei.value.status == FR_ERR_UNSUPPORTED and "a program's ring is read 5 frames back; a streamed block needs delays of at least 64 frames" in str(ei.value)
        assert r.fill_buffer(2, 0, 32, [synth.time_ramp(0, 32)]).shape == (2, 32)
