"""FR_STREAM_PROGRAMS on the GPU: block streaming of plans with stage programs and rings behind one voice bank
(bank_stream_prog_kernel).  Every streamed sample is compared bit for bit with a second HIP renderer that has the option off
and renders the same blocks through fr_fill_buffer, begun with a seek; and with the oracle -- every sample of the small
shapes, sampled frames of the large one.  The serving rule itself: tests/test_stream_plan_sim.py."""
import numpy as np
import pytest

import oracle_tools
import stream_cases as K
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_UNSUPPORTED, RenderError, Renderer, f32_bits
from stream_cases import first_diff, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_IDLE_MS", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# Small shapes, one per patch family, short delays: the rings of a feed-forward plan hold 1024 frames (look-back + a block,
# rounded up to a power of two, at least 1024), so 1500 frames from frame 700 pass every tap's first live frame and wrap the
# rings; the oracle renders every sample.  A feedback plan's rings hold 32768 frames: the small comb goes past that against
# fr_fill_buffer, and against the oracle on its first 1500 frames (the oracle's recursion costs frame / d voices per frame).
SMALL = [
    ("effects", lambda: synth.effects_tree(2, 128, taps=3, base_delay=100.0), 2, 700, 1500, 1500),
    ("envelope_only", lambda: synth.effects_tree(3, 128, taps=0), 3, 300, 1500, 1500),
    ("taps_only", lambda: synth.effects_tree(2, 256, envelope=False, taps=2, base_delay=64.0), 2, 700, 1500, 1500),
    ("comb_64", lambda: K.comb_tree(2, 128, 64), 2, 130, 33500, 1500),
]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("semantics", ["reference", "sparkle"])
@pytest.mark.parametrize("name", [c[0] for c in SMALL])
def test_small_shapes_every_sample(hip_lib, oracle_lib, name, semantics):
    _, build, V, idx0, frames, oracle_frames = K.case(SMALL, name)
    tree = build()
    rng = np.random.default_rng(len(name) * 7919 + V)
    rows = K.block_rows(rng, [(idx0, frames)])
    got, plan = K.stream_against_fill_buffer(hip_lib, tree, V, rows, semantics)
    assert plan["stream"]["servable"] and plan["stream"]["kernel"] == "bank_stream_prog_kernel", plan["stream"]
    ring_frames = 32768 if plan["feedback"] else 1024
    assert frames > ring_frames and frames > plan["max_lookback"]          # the rings wrapped, every tap went live
    with Renderer(oracle_lib, semantics=semantics) as ref:
        synth.install(ref, tree)
        for k, ((idx, row), (_, a)) in enumerate(zip(rows, got)):
            if idx + len(row) > idx0 + oracle_frames:
                break
            exp = ref.fill_buffer(V, idx, idx + len(row), [row])
            assert same_bits(a, exp), f"{name} block {k} at frame {idx} against the oracle: " + first_diff(a, exp)
    assert max(np.nanmax(np.abs(np.where(np.isfinite(a), a, 0))) for _, a in got) > 0.01


@pytest.mark.timeout(900)
@pytest.mark.parametrize("semantics", ["reference", "sparkle"])
@pytest.mark.parametrize("name", ["effects_64x1024", "comb_441"])
def test_large_shapes_sampled_against_oracle(hip_lib, oracle_lib, name, semantics):
    """Config D's patch at 64 x 1024 (four taps reaching 24000 frames back; 4 chunks per voice: 256 workgroups) and the
    16 x 1024 comb: 34000 frames from frame 500 -- every tap live, the 32768-frame rings wrapped --, every sample against
    fr_fill_buffer, and against the oracle's random access on voices x frames: the seek, every tap's first live frame and its
    neighbours, the rings' wrap, the last frame, random ones."""
    _, build, V, _, _ = K.case(K.SERVABLE, name)
    tree = build()
    idx0, frames = 500, 34000
    rng = np.random.default_rng(V)
    rows = K.block_rows(rng, [(idx0, frames)])
    got, plan = K.stream_against_fill_buffer(hip_lib, tree, V, rows, semantics)
    assert plan["stream"]["kernel"] == "bank_stream_prog_kernel"
    # workgroups: 64 voices x 4 chunks of 256 partials; 16 voices x 8 chunks of 128 (a wave needs a group of 8 partials)
    assert plan["stream"]["voices"] * plan["stream"]["chunks"] == (128 if name.startswith("comb") else 256)
    assert frames > 32768 and frames > plan["max_lookback"]
    comb = name.startswith("comb")
    at = [idx0, idx0 + 1, idx0 + 63, idx0 + 64, idx0 + 65, idx0 + 32767, idx0 + 32768, idx0 + frames - 1]
    if comb:   # (the oracle's recursion costs frame / 441 voices per frame: early frames and a few late ones)
        at += [idx0 + 440, idx0 + 441, idx0 + 442, idx0 + 882, idx0 + 4410]
        at = [f for f in at if f < idx0 + 5000] + [idx0 + 32768, idx0 + frames - 1]
        extra = rng.integers(idx0, idx0 + 5000, 8)
    else:
        for tap in (2400, 4800, 7200, 9600, 24000):
            at += [idx0 + tap - 1, idx0 + tap, idx0 + tap + 1]
        extra = rng.integers(idx0, idx0 + frames, 12)
    frames_at = np.unique(np.concatenate([at, extra])).astype(np.uint64)
    voices = np.unique(np.concatenate([[0, 1, V - 1], rng.integers(0, V, 8)])).astype(np.uint32)
    with Renderer(oracle_lib, semantics=semantics) as ref:
        e = tree["edges"]
        synth.install(ref, dict(tree, edges=e[e[:, 1] != 0]))          # (the history goes in before the output edges: nothing is rendered)
        for idx, row in rows:
            assert not ref.fill_buffer(1, idx, idx + len(row), [row]).any()
        ref.on_add_edges(e[e[:, 1] == 0])
        exp = oracle_tools.eval_samples(ref, np.repeat(voices, len(frames_at)), np.tile(frames_at, len(voices))).reshape(len(voices), len(frames_at))
    have = np.empty_like(exp)
    starts = np.array([idx for idx, _ in got])
    for j, f in enumerate(frames_at):
        b = int(np.searchsorted(starts, f, side="right")) - 1
        have[:, j] = got[b][1][voices, int(f) - got[b][0]]
    assert same_bits(have, exp), name + " against the oracle: " + first_diff(have, exp)


@pytest.mark.parametrize("name", ["effects_4x256", "comb_64"])
def test_jumps_forward_and_back_are_seeks(hip_lib, name):
    """A block that does not continue the previous one: the launch is retired, the rings are brought up to the new frame
    and the launch starts there -- what a seek of fr_fill_buffer renders."""
    _, build, V, _, _ = K.case(K.SERVABLE, name)
    rng = np.random.default_rng(5)
    rows = K.block_rows(rng, [(0, 300), (9000, 400), (2500, 300), (2800, 200), (40000, 200), (64, 100)])
    got, plan = K.stream_against_fill_buffer(hip_lib, build(), V, rows)
    assert plan["stream"]["kernel"] == "bank_stream_prog_kernel"


def test_an_edit_ends_the_stream_and_the_next_one_renders_the_new_graph(hip_lib):
    """(The comparison renderer `f` only ever runs while no resident launch does: see stream_cases.stream_against_fill_buffer.)"""
    V, P = 4, 256
    tree = synth.effects_tree(V, P, taps=2, base_delay=200.0)
    rng = np.random.default_rng(9)
    with Renderer(hip_lib, options=K.STREAM_OPTIONS) as s, Renderer(hip_lib) as f:
        synth.install(s, tree)
        synth.install(f, tree)
        idx = 100
        for rnd in range(2):
            s.stream_begin(V)
            rows = K.block_rows(rng, [(idx, 700)])
            got = [s.stream_block(idx_k, row) for idx_k, row in rows]
            idx += 700
            e = tree["edges"]       # an edit: one partial's amplitude (the voices stay template voices)
            amps = tree["params"]["amp"]
            rows_c = np.nonzero((e[:, 0] == synth.CONST_HANDLE) & (e[:, 3] == 0) & np.isin(e[:, 2], synth.bits(amps[amps < 0.4])))[0]
            j = int(rows_c[rng.integers(len(rows_c))])
            new = f32_bits(np.float32(0.25 + 0.01 * rnd))
            s.on_del_edge(synth.CONST_HANDLE, int(e[j, 1]), int(e[j, 2]), 0)
            s.on_add_edge(synth.CONST_HANDLE, int(e[j, 1]), new, 0)
            with pytest.raises(RenderError):
                s.stream_block(idx, synth.time_ramp(idx, idx + 8))        # the edit retired the stream
            # the streamed blocks against fr_fill_buffer of the graph they were rendered from, begun with a seek; then the edit
            for (idx_k, row), a in zip(rows, got):
                b = f.fill_buffer(V, idx_k, idx_k + len(row), [row])
                assert same_bits(a, b), f"round {rnd} frame {idx_k}: " + first_diff(a, b)
            f.on_del_edge(synth.CONST_HANDLE, int(e[j, 1]), int(e[j, 2]), 0)
            f.on_add_edge(synth.CONST_HANDLE, int(e[j, 1]), new, 0)
            e[j, 2] = new
            # an ordinary call after a stream is a seek for the engine (nothing of the stream was stored): so it is for `f`,
            # whose history is dropped by rendering elsewhere first
            row = synth.time_ramp(idx, idx + 100)
            f.fill_buffer(V, 0, 1, [synth.time_ramp(0, 1)])
            assert same_bits(s.fill_buffer(V, idx, idx + 100, [row]), f.fill_buffer(V, idx, idx + 100, [row]))
            idx += 100 + 37                                               # (the next stream starts with a seek again)
        s.stream_begin(V)
        s.stream_end()


@pytest.mark.parametrize("name", [c[0] for c in K.REFUSED])
def test_refusals(hip_lib, name):
    _, build, V, why = K.case(K.REFUSED, name)
    with Renderer(hip_lib, options=K.STREAM_OPTIONS) as r:
        synth.install(r, build())
        with pytest.raises(RenderError) as ei:
            r.stream_begin(V)
        assert ei.value.status == FR_ERR_UNSUPPORTED == 10 and why in str(ei.value), str(ei.value)
        with pytest.raises(RenderError):
            r.stream_block(0, synth.time_ramp(0, 8))                      # no stream open
        t = synth.time_ramp(0, 32)
        assert r.fill_buffer(V, 0, 32, [t]).shape == (V, 32)              # the renderer stays usable


def test_option_off_refuses_programs_as_before(hip_lib):
    with Renderer(hip_lib) as r:
        synth.install(r, synth.effects_tree(4, 256))
        with pytest.raises(RenderError) as ei:
            r.stream_begin(4)
        assert ei.value.status == 10
        assert "block streaming needs a plan that is one voice bank (this one: 1 bank launches, " in str(ei.value) and ", rings" in str(ei.value)
        assert "stream" not in r.plan()


def test_a_bare_bank_streams_through_the_old_kernel(hip_lib, oracle_lib):
    V, P = 3, 512
    tree = synth.additive_tree(V, P)
    rng = np.random.default_rng(3)
    with Renderer(hip_lib, options=K.STREAM_OPTIONS) as s, Renderer(oracle_lib) as ref:
        synth.install(s, tree)
        synth.install(ref, tree)
        s.stream_begin(V)
        for idx, row in K.block_rows(rng, [(0, 600)]):
            assert same_bits(s.stream_block(idx, row), ref.fill_buffer(V, idx, idx + len(row), [row]))
        assert s.plan()["stream"]["kernel"] == "bank_stream_kernel"


# The smallest shapes that reach every step of the resident kernels: one voice of 128 partials (one chunk per voice, one group of
# 8 partials per wave) and two voices of 256 in chunks of 128 (the voice's finisher is whichever chunk arrives last); a full
# block, a block of one frame and a last block of 37; the last voice silent, so that its chunk sums are exact zeros and the
# pass that finds a zero's sign from the leaves runs.  (voices, partials, workgroups)
ZERO_SUM = [(1, 128, 1), (2, 256, 4)]


@pytest.mark.parametrize("V,P,wgs", ZERO_SUM)
@pytest.mark.parametrize("kernel", ["bank_stream_kernel", "bank_stream_prog_kernel"])
def test_a_silent_voice_in_short_blocks(hip_lib, kernel, V, P, wgs):
    tree = synth.additive_tree(V, P) if kernel == "bank_stream_kernel" else synth.effects_tree(V, P, taps=1, base_delay=100.0)
    got, plan = K.stream_against_fill_buffer(hip_lib, K.silence_voice(tree, V, P, V - 1), V, K.short_blocks())
    s = plan["stream"]
    assert s["servable"] and s["kernel"] == kernel and s["voices"] * s["chunks"] == wgs, s
    assert [a.shape for _, a in got] == [(V, 64), (V, 1), (V, 37)]
    assert not any(a[V - 1].any() for _, a in got)                         # the silent voice: zeros of either sign
    assert V == 1 or max(np.abs(a[0]).max() for _, a in got) > 0.01
