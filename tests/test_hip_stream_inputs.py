"""FR_STREAM_INPUTS on the GPU: block streaming of plans whose programs read control rows (bank_stream_in_kernel: a doorbell
of up to 8 rows taken in one look, S_INPUT by row).  The blocks go through fr_stream_block_rows; then, after the stream is
closed (nothing else renders while a launch is resident: stream_cases.stream_against_fill_buffer explains), the same calls go
through fr_fill_buffer of a second HIP renderer with the options off.  Every status must be equal and every sample equal bit
for bit, NaN equal to NaN.  Two cases also run against the oracle directly.  The serving rule: tests/test_stream_inputs_sim.py;
the rows' bookkeeping: tests/test_stream_rows_host.py.

Each test has one streaming renderer at a time."""
import numpy as np
import pytest

import stream_bus_cases as B
import stream_cases as K
import stream_input_cases as I
from libfriendship_amd import synth
from libfriendship_amd.capi import (FR_ERR_INPUT_HISTORY, FR_ERR_INPUT_TOO_LONG, FR_ERR_UNSUPPORTED, FR_OK, RenderError, Renderer)
from stream_cases import first_diff, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_IDLE_MS", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED",
              "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def call(fn):
    try:
        return FR_OK, fn()
    except RenderError as e:
        return e.status, None


def stream_rows_against_fill_buffer(hip_lib, tree, n_rows, blocks, semantics="reference", reference_lib=None):
    """blocks = [(idx, T, rows)] through fr_stream_block_rows, then through fr_fill_buffer of a renderer of `reference_lib`
    (default: the HIP library, options off): equal statuses, equal bits.  Returns [(status, block or None)] and the plan."""
    with Renderer(hip_lib, semantics=semantics, options=I.STREAM_OPTIONS) as s:
        synth.install(s, tree)
        s.stream_begin(n_rows)
        got = [call(lambda: s.stream_block_rows(idx, rows, n_times=T)) for idx, T, rows in blocks]
        plan = s.plan()
        s.stream_end()
    with Renderer(reference_lib or hip_lib, semantics=semantics) as f:
        synth.install(f, tree)
        for k, ((idx, T, rows), (st, a)) in enumerate(zip(blocks, got)):
            st_f, b = call(lambda: f.fill_buffer(n_rows, idx, idx + T, rows))
            assert st == st_f, f"block {k} at frame {idx} (T={T}): status {st} streamed, {st_f} through fr_fill_buffer"
            if st == FR_OK:
                assert same_bits(a, b), f"block {k} at frame {idx} (T={T}, {[len(r) for r in rows]} values): " + first_diff(a, b)
    return got, plan


def loud(got):
    return max(float(np.nanmax(np.abs(np.where(np.isfinite(a), a, 0)))) for st, a in got if st == FR_OK)


@pytest.mark.parametrize("name", [c[0] for c in I.SERVABLE])
def test_every_case_every_sample(hip_lib, name):
    """About 40 blocks of 1..64 frames from frame 300: control rows of every kind (full, short, empty and continuing, constants,
    ramps, +-0, denormals, +-inf, NaN), hostile time values on every fifth block; gated_taps_3x256's taps go live and its
    1024-frame rings wrap."""
    _, build, V, n_rows, slots, per_voice, bus, wgs = I.case(I.SERVABLE, name)
    rng = np.random.default_rng(len(name) * 7919 + V)
    blocks = I.block_inputs(rng, [(300, 1300)], len(slots))
    assert 30 <= len(blocks) <= 60
    got, plan = stream_rows_against_fill_buffer(hip_lib, build(), n_rows, blocks)
    s = plan["stream"]
    assert s["servable"] and s["kernel"] == I.NEW_KERNEL and s["input_slots"] == slots, s
    assert s["programs_per_voice"] == per_voice and s["bus_programs"] == bus and s["voices"] * s["chunks"] == wgs
    assert all(st == FR_OK for st, _ in got) and loud(got) > 0.01


def test_a_seek_in_the_middle(hip_lib):
    """Forward, then back: the launch is retired, the rings are rebuilt with every input 0.0 before the new frame, every slot
    is unfed again -- what a seek of fr_fill_buffer does."""
    rng = np.random.default_rng(11)
    blocks = I.block_inputs(rng, [(300, 400), (9000, 300), (2500, 300)], 2)
    got, plan = stream_rows_against_fill_buffer(hip_lib, I.gated_taps_tree(3, 256), 3, blocks)
    assert plan["stream"]["kernel"] == I.NEW_KERNEL and all(st == FR_OK for st, _ in got) and loud(got) > 0.01


def test_the_vector_count_quirk(hip_lib):
    """One output row, a first block of one frame, three input rows: the store has one vector (slots x frames), so rows 1
    and 2 are dropped and read +0.0; the next block makes room and accepts them."""
    rng = np.random.default_rng(12)
    g = lambda T: rng.uniform(0.5, 1.5, size=T).astype(np.float32)
    blocks = [(500, 1, [synth.time_ramp(500, 501), g(1), g(1)])]
    idx = 501
    for T in (5, 64, 17):
        blocks.append((idx, T, [synth.time_ramp(idx, idx + T), g(T), g(T), g(T), g(T)]))
        idx += T
    got, plan = stream_rows_against_fill_buffer(hip_lib, I.bus_tree(3, 128), 1, blocks)
    assert [st for st, _ in got] == [FR_OK] * 4
    assert not got[0][1].any() and loud(got[1:]) > 0.01


def test_a_slot_left_out_and_fed_again_is_refused(hip_lib):
    rng = np.random.default_rng(13)
    g = lambda T: rng.uniform(0.5, 1.5, size=T).astype(np.float32)
    t = synth.time_ramp
    blocks = [(200, 32, [t(200, 232), g(32), g(32)]),
              (232, 32, [t(232, 264), g(32)]),                      # slot 2 left out: +0.0 in this block
              (264, 32, [t(264, 296), g(32), g(32)]),               # fed again: it holds 232 samples, not 264
              (264, 32, [t(264, 296), g(32)]),                      # the stream is still open and continues
              (4000, 32, [t(4000, 4032), g(32), g(32)])]            # a seek: every slot starts again
    got, plan = stream_rows_against_fill_buffer(hip_lib, I.gain_tree(2, 128), 2, blocks)
    assert [st for st, _ in got] == [FR_OK, FR_OK, FR_ERR_INPUT_HISTORY, FR_OK, FR_OK]
    assert not got[1][1][1].any() and got[1][1][0].any() and got[4][1][1].any()


def test_a_row_longer_than_the_block_is_refused(hip_lib):
    rng = np.random.default_rng(14)
    g = lambda T: rng.uniform(0.5, 1.5, size=T).astype(np.float32)
    t = synth.time_ramp
    blocks = [(100, 16, [t(100, 116), g(16), g(3)]),
              (116, 16, [t(116, 132), g(17), g(16)]),               # n_times + 1 values
              (116, 16, [t(116, 132), np.zeros(0, np.float32), np.zeros(0, np.float32)]),   # continues: padded with block 0's last values
              (132, 7, [t(132, 139), g(7), g(2)])]
    got, plan = stream_rows_against_fill_buffer(hip_lib, I.gain_tree(2, 128), 2, blocks)
    assert [st for st, _ in got] == [FR_OK, FR_ERR_INPUT_TOO_LONG, FR_OK, FR_OK]
    last = [blocks[0][2][1][-1], blocks[0][2][2][-1]]
    assert all(got[2][1][v].any() for v in range(2)) and last[0] != 0 and last[1] != 0


def test_the_one_row_entry_point_reads_the_gains_as_zero(hip_lib):
    """fr_stream_block is fr_stream_block_rows with one row: slots 1 and 2 get none and read +0.0."""
    tree = I.gain_tree(2, 128)
    rows = K.block_rows(np.random.default_rng(15), [(50, 300)])
    with Renderer(hip_lib, options=I.STREAM_OPTIONS) as s:
        synth.install(s, tree)
        s.stream_begin(2)
        got = [s.stream_block(idx, row) for idx, row in rows]
        assert s.plan()["stream"]["kernel"] == I.NEW_KERNEL
        s.stream_end()
    with Renderer(hip_lib) as f:
        synth.install(f, tree)
        for (idx, row), a in zip(rows, got):
            b = f.fill_buffer(2, idx, idx + len(row), [row])
            assert same_bits(a, b), f"frame {idx}: " + first_diff(a, b)


@pytest.mark.parametrize("semantics", ["reference", "sparkle"])
@pytest.mark.parametrize("name", ["gain_2x128", "bus_3x128"])
def test_against_the_oracle(hip_lib, oracle_lib, name, semantics):
    _, build, V, n_rows, slots, _, _, _ = I.case(I.SERVABLE, name)
    rng = np.random.default_rng(len(name) + len(semantics))
    blocks = I.block_inputs(rng, [(700, 8 * 64)], len(slots))[:8]
    got, plan = stream_rows_against_fill_buffer(hip_lib, build(), n_rows, blocks, semantics, reference_lib=oracle_lib)
    assert plan["stream"]["kernel"] == I.NEW_KERNEL and all(st == FR_OK for st, _ in got) and loud(got) > 0.01


def test_without_the_option_the_patch_is_refused_as_before(hip_lib):
    with Renderer(hip_lib, options=B.STREAM_OPTIONS) as r:
        synth.install(r, I.gain_tree(2, 128))
        with pytest.raises(RenderError) as ei:
            r.stream_begin(2)
        assert ei.value.status == FR_ERR_UNSUPPORTED and "a program reads input slot 1; " + I.OLD_REASON in str(ei.value), str(ei.value)
        assert r.fill_buffer(2, 0, 32, [synth.time_ramp(0, 32)]).shape == (2, 32)      # the renderer stays usable


def test_a_plan_that_reads_slot_0_only_keeps_its_kernel(hip_lib):
    _, build, V, per_voice, _ = K.case(K.SERVABLE, "effects_2x128")
    rows = K.block_rows(np.random.default_rng(16), [(50, 400)])
    got, plan = B.stream_against_fill_buffer(hip_lib, build(), V, rows, options=I.STREAM_OPTIONS)
    s = plan["stream"]
    assert s["kernel"] == "bank_stream_prog_kernel" and s["input_slots"] == [0] and s["programs_per_voice"] == [per_voice] * V


@pytest.mark.parametrize("V,P,wgs", [(1, 128, 1), (2, 256, 4)])
def test_a_silent_voice_in_short_blocks(hip_lib, V, P, wgs):
    """One voice of one chunk (one group of 8 partials per wave) and two voices of two chunks each; a full block, a block of
    one frame and a last block of 37; the last voice silent: its chunk sums are exact zeros, whose sign the kernel finds from
    the leaves.  Row v = voice v x its gain row."""
    tree = K.silence_voice(I.gain_tree(V, P), V, P, V - 1)
    rng = np.random.default_rng(V)
    blocks = [(idx, len(t), [t] + [rng.uniform(0.5, 1.5, size=len(t)).astype(np.float32) for _ in range(V)]) for idx, t in K.short_blocks()]
    got, plan = stream_rows_against_fill_buffer(hip_lib, tree, V, blocks)
    s = plan["stream"]
    assert s["servable"] and s["kernel"] == I.NEW_KERNEL and s["voices"] * s["chunks"] == wgs, s
    assert [st for st, _ in got] == [FR_OK] * 3 and [a.shape for _, a in got] == [(V, 64), (V, 1), (V, 37)]
    assert not any(a[V - 1].any() for _, a in got) and (V == 1 or loud(got) > 0.01)
