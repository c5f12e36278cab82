"""FR_STREAM_GENERAL on the GPU: block streaming of voices of any partial count (bank_stream_general_kernel: one workgroup per
schedule voice runs the voice's items on its 16 waves and the merges on wave 0's LDS stack).  Blocks go through
fr_stream_block_rows from frame 0; then, after the stream is closed (nothing else renders while a launch is resident), the same
blocks go through fr_fill_buffer of a second HIP renderer with no stream option set -- every sample equal bit for bit, NaN equal
to NaN, +0 unequal to -0 -- and the first blocks, up to the frame the case's leaf budget gives, through the oracle; then the
plan's "stream" object.  The serving rule: tests/test_stream_general_sim.py; the schedule validation and a host model of the
schedule renderer: tests/test_stream_general_host.py.

Each test has one streaming renderer at a time.  A block that is not answered ends the stream within the engine's own bounds
(250 ms per block, FR_STREAM_IDLE_MS for the launch)."""
import numpy as np
import pytest

import stream_general_cases as G
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_UNSUPPORTED, RenderError, Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_LOOP_TILES", "FR_STREAM_IDLE_MS",
              "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def trees():
    return {}


def tree_of(trees, name):
    if name not in trees:
        trees[name] = G.case(name)["build"]()
    return trees[name]


def loud(got):
    return max(float(np.nanmax(np.abs(np.where(np.isfinite(a), a, 0)))) for a in got)


def run_case(hip_lib, oracle_lib, tree, c, blocks, semantics="reference", oracle=True):
    """Streamed, then every sample against fr_fill_buffer, then the early blocks against the oracle, then the plan; returns it."""
    got, plan = G.stream_all(hip_lib, tree, c["n_rows"], blocks, c["options"], semantics)
    frames = sum(T for _, T, _ in blocks)
    assert G.fill_compare(hip_lib, tree, c["n_rows"], blocks, got, "through fr_fill_buffer", semantics) == frames
    if oracle:
        assert blocks[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
        assert G.fill_compare(oracle_lib, tree, c["n_rows"], blocks, got, "on the oracle", semantics, upto=c["oracle_frames"]) == min(frames, c["oracle_frames"])
    G.check_stream_object(plan["stream"], c)
    assert loud(got) > 0.01
    return plan


@pytest.mark.parametrize("name", [c["name"] for c in G.SERVABLE])
def test_every_case_every_sample(hip_lib, oracle_lib, trees, name):
    """About 1500 frames from frame 0 in blocks of random length 1..64, every fifth time row hostile (negative, above 2^32, NaN,
    infinite: the workgroup leaves the fast path); control rows of every kind."""
    c = G.case(name)
    rng = np.random.default_rng(len(name) * 7919)
    blocks = G.blocks_of(G.block_rows(rng, [(0, 1500)]), rng, c["n_in"])
    run_case(hip_lib, oracle_lib, tree_of(trees, name), c, blocks)


@pytest.mark.parametrize("P", [100, 129])
def test_short_blocks_with_a_silent_voice(hip_lib, oracle_lib, P):
    """A full block, a block of one frame and a block of 37 from frame 0, the last voice silent: every root of it is an exact
    zero, so the sign pass runs on all lanes -- the split items on their waves, the padded group and the single leaf on wave 0."""
    c = G.case(f"additive_2x{P}")
    tree = G.silence_voice(c["build"](), 2, P, 1)
    blocks = G.blocks_of(G.short_blocks(idx=0))
    got, plan = G.stream_all(hip_lib, tree, 2, blocks, c["options"])
    assert G.fill_compare(hip_lib, tree, 2, blocks, got, "through fr_fill_buffer") == 102
    assert G.fill_compare(oracle_lib, tree, 2, blocks, got, "on the oracle") == 102
    G.check_stream_object(plan["stream"], c)
    assert [a.shape for a in got] == [(2, 64), (2, 1), (2, 37)]
    assert not any(a[1].any() for a in got) and loud(got) > 0.01       # zeros (their signs: the two comparisons above)


@pytest.mark.parametrize("name", ["additive_2x100", "comb_5_2x100"])
def test_jumps_are_seeks(hip_lib, trees, name):
    """A block that does not continue the previous one retires the launch; the next one starts at the new frame."""
    c = G.case(name)
    starts = [(0, 300), (9000, 200), (2500, 200), (40000, 100), (64, 100)]
    blocks = G.blocks_of(G.block_rows(np.random.default_rng(len(name)), starts))
    run_case(hip_lib, None, tree_of(trees, name), c, blocks, oracle=False)


def test_sparkle_semantics(hip_lib, oracle_lib, trees):
    c = G.case("comb_5_2x100")
    rng = np.random.default_rng(11)
    blocks = G.blocks_of(G.block_rows(rng, [(0, 700)]), rng, c["n_in"])
    run_case(hip_lib, oracle_lib, tree_of(trees, c["name"]), c, blocks, semantics="sparkle")


def test_without_the_option_a_general_voice_is_refused_as_before(hip_lib, trees):
    tree = tree_of(trees, "additive_2x100")
    with Renderer(hip_lib, options=dict(G.PROGRAMS, **G.IDLE)) as r:
        synth.install(r, tree)
        r.fill_buffer(2, 0, 32, [synth.time_ramp(0, 32)])
        assert r.plan()["stream"]["reason"] == G.OLD_GENERAL
        with pytest.raises(RenderError) as ei:
            r.stream_begin(2)
        assert ei.value.status == FR_ERR_UNSUPPORTED and "block streaming needs balanced template voices" in str(ei.value)
        assert r.fill_buffer(2, 32, 64, [synth.time_ramp(32, 64)]).shape == (2, 32)


def test_balanced_voices_of_128_keep_their_kernel(hip_lib):
    """2 x 128 balanced with the option on: no schedule bank, the kernel it has today."""
    tree = synth.additive_tree(2, 128)
    blocks = G.blocks_of(G.block_rows(np.random.default_rng(128), [(0, 400)]))
    got, plan = G.stream_all(hip_lib, tree, 2, blocks, G.OPTION)
    s = plan["stream"]
    assert s["servable"] and s["kernel"] in ("bank_stream_prog_kernel", "bank_stream_kernel") and s["general_voices"] == [], s
    assert G.fill_compare(hip_lib, tree, 2, blocks, got, "through fr_fill_buffer") == 400
