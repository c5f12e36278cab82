"""FR_STREAM_BUS on the GPU: block streaming of plans whose programs mix several voices of a block (bank_stream_bus_kernel:
the wave that counts the block's last voice in runs the bus programs before it writes the done tag).  Every streamed sample
is compared bit for bit with a second HIP renderer that has both options off and renders the same blocks through
fr_fill_buffer after the stream is closed; and with the oracle -- every sample of the small shapes, sampled frames of the
large one.  The serving rule itself: tests/test_stream_bus_sim.py.

Each test has one streaming renderer at a time, and nothing else renders while its launch is resident."""
import numpy as np
import pytest

import oracle_tools
import stream_bus_cases as B
import stream_cases as K
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_UNSUPPORTED, RenderError, Renderer, f32_bits
from stream_cases import first_diff, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_IDLE_MS", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# The smallest shapes at which each mechanism can go wrong.  (name, builder, voices, rows, first frame, frames, frames
# against the oracle, workgroups.)  A feed-forward plan's rings hold 1024 frames (look-back + a block, rounded up to a power of
# two, at least 1024): 1500 frames from frame 700 pass every tap's first live frame and wrap the rings.  A feedback plan's
# rings hold 32768 frames: the comb goes past that against fr_fill_buffer, and against the oracle on its first 1500 frames
# (the oracle's recursion costs frame / d buses per frame).
SMALL = [
    ("mix_2x128", lambda: B.mixdown_tree(2, 128, 1), 2, 1, 700, 1500, 1500, 2),                       # the smallest bus
    ("mix_3x128", lambda: B.mixdown_tree(3, 128, 1), 3, 1, 700, 1500, 1500, 3),                       # an odd voice count
    ("mix_2x128_env", lambda: B.mixdown_tree(2, 128, 1, envelope=True), 2, 1, 300, 1500, 1500, 2),    # S_INPUT in a bus program
    ("mix_4x128_2_pre", lambda: B.mixdown_tree(4, 128, 2, pre_taps=1, base_delay=100.0), 4, 2, 700, 1500, 1500, 4),
    ("mix_4x128_2_post", lambda: B.mixdown_tree(4, 128, 2, post_taps=1, base_delay=64.0), 4, 2, 700, 1500, 1500, 4),  # a bus ring one block back
    ("rows_and_bus_3x128", lambda: B.rows_and_bus_tree(3, 128), 3, 4, 300, 1500, 1500, 3),            # voice programs and a bus
    ("bus_comb_64", lambda: B.bus_comb_tree(2, 128, 64), 2, 1, 130, 33500, 1500, 2),
    ("mix_2x1024", lambda: B.mixdown_tree(2, 1024, 1), 2, 1, 700, 1500, 1500, 16),                    # chunked voices: finisher and last arriver move
]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("semantics", ["reference", "sparkle"])
@pytest.mark.parametrize("name", [c[0] for c in SMALL])
def test_small_shapes_every_sample(hip_lib, oracle_lib, name, semantics):
    _, build, V, n_rows, idx0, frames, oracle_frames, wgs = K.case(SMALL, name)
    tree = build()
    rng = np.random.default_rng(len(name) * 7919 + V)
    rows = K.block_rows(rng, [(idx0, frames)])
    got, plan = B.stream_against_fill_buffer(hip_lib, tree, n_rows, rows, semantics)
    s = plan["stream"]
    assert s["servable"] and s["kernel"] == "bank_stream_bus_kernel" and s["bus_programs"] >= 1, s
    assert s["voices"] == V and s["voices"] * s["chunks"] == wgs
    ring_frames = 32768 if plan["feedback"] else 1024
    assert frames > ring_frames and frames > plan["max_lookback"]          # the rings wrapped, every tap went live
    with Renderer(oracle_lib, semantics=semantics) as ref:
        synth.install(ref, tree)
        for k, ((idx, row), (_, a)) in enumerate(zip(rows, got)):
            if idx + len(row) > idx0 + oracle_frames:
                break
            exp = ref.fill_buffer(n_rows, idx, idx + len(row), [row])
            assert same_bits(a, exp), f"{name} block {k} at frame {idx} against the oracle: " + first_diff(a, exp)
    for r in range(n_rows):                                                 # no row is silent
        assert max(np.nanmax(np.abs(np.where(np.isfinite(a[r]), a[r], 0))) for _, a in got) > 0.01


@pytest.mark.timeout(900)
def test_64_voices_to_two_buses(hip_lib, oracle_lib):
    """64 x 256 -> 2: 128 workgroups (2 chunks per voice), each bus program sums 32 voices.  1500 frames from frame 500 -- the
    1024-frame rings wrap --, every sample against fr_fill_buffer; against the oracle's random access both rows at the seek,
    frames 63 / 64 / 65, the rings' wrap and the last frame."""
    V, n_rows = 64, 2
    tree = B.mixdown_tree(V, 256, n_rows)
    idx0, frames = 500, 1500
    rng = np.random.default_rng(V)
    rows = K.block_rows(rng, [(idx0, frames)])
    got, plan = B.stream_against_fill_buffer(hip_lib, tree, n_rows, rows)
    s = plan["stream"]
    assert s["kernel"] == "bank_stream_bus_kernel" and s["bus_programs"] == 2 and s["programs_per_voice"] == [0] * V
    assert s["voices"] * s["chunks"] == 128
    assert not plan["feedback"] and frames > 1024
    frames_at = np.array([idx0, idx0 + 1, idx0 + 63, idx0 + 64, idx0 + 65, idx0 + 1023, idx0 + 1024, idx0 + 1025, idx0 + frames - 1], np.uint64)
    slots = np.arange(n_rows, dtype=np.uint32)
    with Renderer(oracle_lib) as ref:
        e = tree["edges"]
        synth.install(ref, dict(tree, edges=e[e[:, 1] != 0]))          # (the history goes in before the output edges: nothing is rendered)
        for idx, row in rows:
            assert not ref.fill_buffer(1, idx, idx + len(row), [row]).any()
        ref.on_add_edges(e[e[:, 1] == 0])
        exp = oracle_tools.eval_samples(ref, np.repeat(slots, len(frames_at)), np.tile(frames_at, n_rows)).reshape(n_rows, len(frames_at))
    have = np.empty_like(exp)
    starts = np.array([idx for idx, _ in got])
    for j, f in enumerate(frames_at):
        b = int(np.searchsorted(starts, f, side="right")) - 1
        have[:, j] = got[b][1][:, int(f) - got[b][0]]
    assert same_bits(have, exp), "against the oracle: " + first_diff(have, exp)
    assert all(max(np.nanmax(np.abs(np.where(np.isfinite(a[r]), a[r], 0))) for _, a in got) > 0.01 for r in range(n_rows))


def test_jumps_forward_and_back_are_seeks(hip_lib):
    """A block that does not continue the previous one: the launch is retired, the rings are brought up to the new frame
    and the launch starts there -- what a seek of fr_fill_buffer renders."""
    rng = np.random.default_rng(5)
    rows = K.block_rows(rng, [(0, 300), (9000, 400), (2500, 300), (2800, 200), (40000, 200), (64, 100)])
    got, plan = B.stream_against_fill_buffer(hip_lib, B.mixdown_tree(4, 128, 2, pre_taps=1, base_delay=100.0), 2, rows)
    assert plan["stream"]["kernel"] == "bank_stream_bus_kernel"


def test_an_edit_ends_the_stream_and_the_next_one_renders_the_new_graph(hip_lib):
    """(The comparison renderer `f` only ever runs while no resident launch does.)"""
    V, n_rows = 4, 2
    tree = B.mixdown_tree(V, 128, n_rows, post_taps=1, base_delay=200.0)
    rng = np.random.default_rng(9)
    e = tree["edges"]
    # the edit: voice 1's gain (a constant of a bus program; the voices stay template voices)
    j = int(np.nonzero((e[:, 0] == synth.CONST_HANDLE) & (e[:, 3] == 0) & (e[:, 2] == synth.bits(B.gains(V)[1])))[0][0])
    with Renderer(hip_lib, options=B.STREAM_OPTIONS) as s, Renderer(hip_lib) as f:
        synth.install(s, tree)
        synth.install(f, tree)
        idx = 100
        for rnd in range(2):
            s.stream_begin(n_rows)
            rows = K.block_rows(rng, [(idx, 700)])
            got = [s.stream_block(idx_k, row) for idx_k, row in rows]
            assert s.plan()["stream"]["kernel"] == "bank_stream_bus_kernel"
            idx += 700
            new = f32_bits(np.float32(0.3 + 0.05 * rnd))
            s.on_del_edge(synth.CONST_HANDLE, int(e[j, 1]), int(e[j, 2]), 0)
            s.on_add_edge(synth.CONST_HANDLE, int(e[j, 1]), new, 0)
            with pytest.raises(RenderError):
                s.stream_block(idx, synth.time_ramp(idx, idx + 8))        # the edit retired the stream
            # the streamed blocks against fr_fill_buffer of the graph they were rendered from, begun with a seek; then the edit
            for (idx_k, row), a in zip(rows, got):
                b = f.fill_buffer(n_rows, idx_k, idx_k + len(row), [row])
                assert same_bits(a, b), f"round {rnd} frame {idx_k}: " + first_diff(a, b)
            f.on_del_edge(synth.CONST_HANDLE, int(e[j, 1]), int(e[j, 2]), 0)
            f.on_add_edge(synth.CONST_HANDLE, int(e[j, 1]), new, 0)
            e[j, 2] = new
            # an ordinary call after a stream is a seek for the engine (nothing of the stream was stored): so it is for `f`,
            # whose history is dropped by rendering elsewhere first
            row = synth.time_ramp(idx, idx + 100)
            f.fill_buffer(n_rows, 0, 1, [synth.time_ramp(0, 1)])
            assert same_bits(s.fill_buffer(n_rows, idx, idx + 100, [row]), f.fill_buffer(n_rows, idx, idx + 100, [row]))
            idx += 100 + 37                                               # (the next stream starts with a seek again)
        s.stream_begin(n_rows)
        s.stream_end()


def test_without_the_bus_option_the_mix_is_refused_and_the_renderer_stays_usable(hip_lib):
    with Renderer(hip_lib, options=K.STREAM_OPTIONS) as r:
        synth.install(r, B.mixdown_tree(4, 128, 2))
        with pytest.raises(RenderError) as ei:
            r.stream_begin(2)
        assert ei.value.status == FR_ERR_UNSUPPORTED and "mix bus" in str(ei.value), str(ei.value)
        t = synth.time_ramp(0, 32)
        assert r.fill_buffer(2, 0, 32, [t]).shape == (2, 32)


def test_a_plan_without_a_bus_keeps_its_kernel(hip_lib):
    """With both options on, per-voice programs alone still run bank_stream_prog_kernel."""
    V = 2
    tree = synth.effects_tree(V, 128, taps=1, base_delay=100.0)
    rows = K.block_rows(np.random.default_rng(2), [(50, 400)])
    got, plan = B.stream_against_fill_buffer(hip_lib, tree, V, rows)
    assert plan["stream"]["kernel"] == "bank_stream_prog_kernel" and plan["stream"]["bus_programs"] == 0


@pytest.mark.parametrize("P,wgs", [(128, 2), (256, 4)])
def test_a_silent_voice_in_short_blocks(hip_lib, P, wgs):
    """Two voices (a bus has at least two) of one chunk and of two chunks each; a full block, a block of one frame and a last
    block of 37; voice 1 silent: its chunk sums are exact zeros, whose sign the kernel finds from the leaves.  Rows 0 and 1 are
    the voices, row 2 their mix."""
    V = 2
    tree = K.silence_voice(B.rows_and_bus_tree(V, P), V, P, 1)
    got, plan = B.stream_against_fill_buffer(hip_lib, tree, V + 1, K.short_blocks())
    s = plan["stream"]
    assert s["servable"] and s["kernel"] == "bank_stream_bus_kernel" and s["bus_programs"] == 1 and s["voices"] * s["chunks"] == wgs, s
    assert [a.shape for _, a in got] == [(V + 1, 64), (V + 1, 1), (V + 1, 37)]
    assert not any(a[1].any() for _, a in got) and max(np.abs(a[2]).max() for _, a in got) > 0.01
