"""FR_STREAM_DYN on the GPU: block streaming of Delays by a signal amount (bank_stream_dyn_kernel: the general kernel's
composition with an interpreter that knows S_READ_DYN and S_STEP_DYN).  Blocks go through fr_stream_block_rows; then, after the
stream is closed (nothing else renders while a launch is resident), the same blocks go through fr_fill_buffer of a second HIP
renderer with no stream option set -- every sample equal bit for bit, NaN equal to NaN, +0 unequal to -0 -- and the first blocks,
up to the frame the case's leaf budget gives, through the oracle; then the plan's "stream" object.  The rings are sized and
warmed up by what sizes and warms them for any other plan: the seeks below land where only the bound's look-back explains the
samples.  The serving rule: tests/test_stream_dyn_sim.py; the rule on hand-built plans, the launch rule and a host model of the
two ops: tests/test_stream_dyn_host.py.

Each test has one streaming renderer at a time.  A block that is not answered ends the stream within the engine's own bounds
(250 ms per block, FR_STREAM_IDLE_MS for the launch)."""
import numpy as np
import pytest

import stream_cases as K
import stream_dyn_cases as D
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_UNSUPPORTED, RenderError, Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN", "FR_LOOP_TILES",
              "FR_STREAM_IDLE_MS", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def trees():
    return {}


def tree_of(trees, name):
    if name not in trees:
        trees[name] = D.case(name)["build"]()
    return trees[name]


def loud(got):
    return max(float(np.nanmax(np.abs(np.where(np.isfinite(a), a, 0)))) for a in got)


def blocks_for(c, rng, starts):
    """Blocks of random length 1..64, every fifth time row hostile; control rows of every kind, scaled to amounts for the knobs."""
    blocks = D.blocks_of(D.block_rows(rng, starts), rng, c["n_in"])
    return D.knob_blocks(blocks) if c["n_in"] > 1 else blocks


def run_case(hip_lib, oracle_lib, tree, c, blocks, semantics="reference", oracle=True):
    """Streamed, then every sample against fr_fill_buffer, then the early blocks against the oracle, then the plan; returns the blocks' results."""
    got, plan = D.stream_all(hip_lib, tree, c["n_rows"], blocks, c["options"], semantics)
    frames = sum(T for _, T, _ in blocks)
    assert D.fill_compare(hip_lib, tree, c["n_rows"], blocks, got, "through fr_fill_buffer", semantics) == frames
    if oracle:
        assert blocks[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
        assert D.fill_compare(oracle_lib, tree, c["n_rows"], blocks, got, "on the oracle", semantics, upto=c["oracle_frames"]) == min(frames, c["oracle_frames"])
    D.check_stream_object(plan["stream"], c)
    assert loud(got) > 0.01
    return got


@pytest.mark.parametrize("name", [c["name"] for c in D.SERVABLE])
def test_every_case_every_sample(hip_lib, oracle_lib, trees, name):
    """About 1500 frames from frame 0 in blocks of random length 1..64, every fifth time row hostile (negative, above 2^32, NaN,
    infinite: the amount of a chorus follows them), control rows of every kind (the knob: negative, fractional, NaN, +-inf,
    above its 48)."""
    c = D.case(name)
    rng = np.random.default_rng(len(name) * 7919)
    run_case(hip_lib, oracle_lib, tree_of(trees, name), c, blocks_for(c, rng, [(0, 1500)]))


def test_short_blocks_with_a_silent_voice(hip_lib, oracle_lib):
    """A full block, a block of one frame and a block of 37 from frame 0, the last voice silent: its ring holds zeros whose
    signs the signal read hands on."""
    c = D.case("chorus_short")
    tree = D.silence_voice(c["build"](), 2, 128, 1)
    blocks = D.blocks_of(D.short_blocks(idx=0))
    got, plan = D.stream_all(hip_lib, tree, 2, blocks, c["options"])
    assert D.fill_compare(hip_lib, tree, 2, blocks, got, "through fr_fill_buffer") == 102
    assert D.fill_compare(oracle_lib, tree, 2, blocks, got, "on the oracle") == 102
    D.check_stream_object(plan["stream"], c)
    assert [a.shape for a in got] == [(2, 64), (2, 1), (2, 37)]
    assert not any(a[1].any() for a in got) and loud(got) > 0.01       # zeros (their signs: the two comparisons above)


@pytest.mark.parametrize("name", ["chorus_2x128", "chorus_short"])
def test_jumps_are_seeks(hip_lib, trees, name):
    """A block that does not continue the previous one retires the launch; the warm-up fills the rings for the bound's look-back
    (700 frames: a block at 9000 reads frames 8300..8600 that no block of this stream rendered)."""
    c = D.case(name)
    starts = [(0, 300), (9000, 200), (2500, 200), (40000, 100), (64, 100)]
    blocks = blocks_for(c, np.random.default_rng(len(name)), starts)
    run_case(hip_lib, None, tree_of(trees, name), c, blocks, oracle=False)


def test_sparkle_semantics(hip_lib, oracle_lib, trees):
    """SparkleRenderer's cast: a negative or NaN amount gives 0.0 where the reference delays by 0 frames."""
    c = D.case("chorus_zero")
    rng = np.random.default_rng(11)
    run_case(hip_lib, oracle_lib, tree_of(trees, c["name"]), c, blocks_for(c, rng, [(0, 700)]), semantics="sparkle")
    c = D.case("knob")
    tree = tree_of(trees, c["name"])
    blocks = blocks_for(c, rng, [(0, 700)])
    got = run_case(hip_lib, oracle_lib, tree, c, blocks, semantics="sparkle")
    # sparkle: where the knob is negative or NaN the row is the voice + 0.0 (a NaN on Minimum's left wins there: Minimum(NaN, 48)
    # delaying by 48 frames would be heard); the reference's cast makes a negative amount 0 frames: the voice + the voice
    ref = run_case(hip_lib, oracle_lib, tree, c, blocks)
    assert any(np.isnan(rows[1]).any() for _, _, rows in blocks) and any((rows[1] < 0).any() for _, _, rows in blocks)
    with Renderer(oracle_lib) as o, np.errstate(all="ignore"):
        synth.install(o, D.dry_tree(2, 128))
        for (idx, T, rows), a, b in zip(blocks, got, ref):
            dry = o.fill_buffer(2, idx, idx + T, [rows[0]])
            neg = rows[1] < 0
            m = neg | np.isnan(rows[1])
            assert K.same_bits(a[:, m], (dry + np.float32(0.0))[:, m]), f"sparkle, block at {idx}: " + K.first_diff(a[:, m], (dry + np.float32(0.0))[:, m])
            assert K.same_bits(b[:, neg], (dry + dry)[:, neg]), f"reference, block at {idx}: " + K.first_diff(b[:, neg], (dry + dry)[:, neg])


def test_without_the_option_a_chorus_is_refused_as_before(hip_lib, trees):
    tree = tree_of(trees, "chorus_2x128")
    with Renderer(hip_lib, options=dict(D.PROGRAMS, **D.IDLE)) as r:
        synth.install(r, tree)
        r.fill_buffer(2, 0, 32, [synth.time_ramp(0, 32)])
        s = r.plan()["stream"]
        assert s["reason"] == D.OLD_REASON and not any(k in s for k in D.NEW_KEYS)
        with pytest.raises(RenderError) as ei:
            r.stream_begin(2)
        assert ei.value.status == FR_ERR_UNSUPPORTED and D.OLD_REASON in str(ei.value)
        assert r.fill_buffer(2, 32, 64, [synth.time_ramp(32, 64)]).shape == (2, 32)


def test_a_plan_without_a_signal_delay_keeps_its_kernel(hip_lib):
    """2 x 128 balanced with the option on: no signal delay, the kernel it has today and the same samples."""
    tree = synth.additive_tree(2, 128)
    blocks = D.blocks_of(D.block_rows(np.random.default_rng(128), [(0, 400)]))
    a, plan_a = D.stream_all(hip_lib, tree, 2, blocks, D.PROGRAMS)
    b, plan_b = D.stream_all(hip_lib, tree, 2, blocks, D.OPTION)
    s = plan_b["stream"]
    assert s["servable"] and s["kernel"] == plan_a["stream"]["kernel"] and s["kernel"] in ("bank_stream_prog_kernel", "bank_stream_kernel") and s["dyn_reads"] == 0 and s["dyn_steps"] == 0, s
    assert all(K.same_bits(x, y) for x, y in zip(a, b))
    assert D.fill_compare(hip_lib, tree, 2, blocks, b, "through fr_fill_buffer") == 400
