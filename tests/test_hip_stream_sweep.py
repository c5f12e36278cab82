"""FR_STREAM_SWEEP on the MI355X: the four sweep kernels (bank_stream_sweep_kernel, _fx, _store, _store_fx; csrc/kernels.hpp).

Every servable case of tests/stream_sweep_cases.py is streamed from frame 0 in blocks of 1..64 frames (1500 frames), and every
streamed sample is compared bit for bit (NaN equal to NaN, +0 unequal to -0)
  * with fr_fill_buffer of the same blocks on a second HIP renderer with FR_LOOP_DYN=1 and no stream option,
  * for the voiceless cases with the dense forward reference (tests/loop_dyn_reference.py) on every frame,
  * with the C++ oracle up to the case's `oracle` frame count.
Further: blocks of 64, 1 and 37 frames from frame 0; jumps as seeks at w = 1 and 7; 33 500 frames at w = 7 (the rings wrap many
times); the Sparkle semantics on the flanger of base 8; and the two store forms with an edit of the feedback gain between two
blocks -- what follows must equal the fr_fill_buffer twin given the same edit.  Without the feature every one of these streams is
refused by fr_stream_begin.

tests/test_stream_sweep_sim.py has proven on the CPU that every expected row is at least 95 % finite and audible.  One streaming
renderer at a time; the twin renders after the stream is closed."""
import numpy as np
import pytest

import stream_cases as K
import stream_sweep_cases as S
from libfriendship_amd.capi import Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_LOOP_DYN", "FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN",
              "FR_STREAM_HISTORY", "FR_STREAM_EFFECTS", "FR_STREAM_STORE", "FR_STREAM_TAPS", "FR_STREAM_SWEEP", "FR_LOOP_TILES", "FR_STREAM_IDLE_MS", "FR_RING_KEEP",
              "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def oracle_rows(oracle_lib, p, blocks, semantics=None):
    m = p.oracle
    rows = [r[:m] for r in S.concat_rows(blocks)]
    with Renderer(oracle_lib, semantics=semantics or p.semantics) as o:
        p.install(o)
        return o.fill_buffer(p.n_rows, 0, m, rows)


def stream_and_compare(hip_lib, oracle_lib, p, blocks, key, semantics=None, oracle=True, dense=True):
    """Streams the blocks, checks the "stream" object and compares three ways; returns the frames compared with each."""
    got, first, last = S.stream_blocks(hip_lib, p, blocks, semantics=semantics)
    S.check_stream_object(first, p)
    assert last["kernel"] == p.kernel(), last
    twin = S.fill_blocks(hip_lib, p, blocks, semantics=semantics)
    n = S.compare_blocks(got, twin, blocks, f"{p.name} [{key}], streamed against fr_fill_buffer")
    all_got = np.concatenate(got, axis=1)
    n_dense = n_oracle = 0
    if dense and p.voiceless:
        exp = S.dense_reference(p, blocks, key) if semantics is None else None
        if exp is None:
            import loop_dyn_reference as ldr
            rows = S.concat_rows(blocks)
            exp = ldr.render(p.build(), rows, 0, len(rows[0]), semantics)
        assert K.same_bits(all_got, exp), f"{p.name} [{key}], streamed against the dense forward reference: " + K.first_diff(all_got, exp)
        n_dense = exp.shape[1]
    if oracle:
        exp = oracle_rows(oracle_lib, p, blocks, semantics)
        m = exp.shape[1]
        assert K.same_bits(all_got[:, :m], exp), f"{p.name} [{key}], streamed against the oracle on frames 0..{m - 1}: " + K.first_diff(all_got[:, :m], exp)
        n_oracle = m
    fin = np.isfinite(all_got)
    assert fin.mean(axis=1).min() >= S.FINITE_SHARE and np.abs(np.where(fin, all_got, 0)).max(axis=1).min() > S.LOUD
    print(f"{p.name} [{key}]: {n} frames compared with fr_fill_buffer, {n_dense} with the dense reference, {n_oracle} with the oracle; {last['kernel']}")
    return n, n_dense, n_oracle


@pytest.mark.parametrize("p", S.SERVABLE, ids=S.IDS)
def test_every_streamed_sample(hip_lib, oracle_lib, p):
    blocks = S.blocks_of(p, [(0, S.FRAMES)])
    n, n_dense, n_oracle = stream_and_compare(hip_lib, oracle_lib, p, blocks, "main")
    assert n == S.FRAMES and n_oracle == p.oracle and n_dense == (S.FRAMES if p.voiceless else 0)


@pytest.mark.parametrize("name", ["flanger_2_3", "flanger_8", "flanger_64", "voices_base_8", "chorus_comb"])
def test_short_blocks_from_frame_0(hip_lib, oracle_lib, name):
    p = S.case(name)
    blocks = S.short_blocks_of(p)
    assert [T for _, T, _ in blocks] == [64, 1, 37]
    stream_and_compare(hip_lib, oracle_lib, p, blocks, "short", oracle=False)


@pytest.mark.parametrize("name", S.SEEK_CASES)
def test_jumps_are_seeks(hip_lib, name):
    """[(0, 300), (9000, 200), (2500, 200)]: a block that does not continue the previous one retires the launch and replays by the
    ordinary path; the streamed blocks equal fr_fill_buffer's, which seeks at the same frames."""
    p = S.case(name)
    blocks = S.blocks_of(p, S.SEEKS, seed=31)
    got, first, last = S.stream_blocks(hip_lib, p, blocks)
    S.check_stream_object(last, p)
    twin = S.fill_blocks(hip_lib, p, blocks)
    assert S.compare_blocks(got, twin, blocks, f"{name}, seeks, streamed against fr_fill_buffer") == 700


def test_rings_wrap(hip_lib):
    """33 500 frames at w = 7 in blocks of 1..64 frames: every sample against the dense forward reference and against fr_fill_buffer
    in calls of 4 800 frames."""
    p = S.case("flanger_8")
    blocks = S.blocks_of(p, [(0, S.WRAP_FRAMES)], seed=41)
    got, first, last = S.stream_blocks(hip_lib, p, blocks)
    S.check_stream_object(last, p)
    all_got = np.concatenate(got, axis=1)
    exp = S.dense_reference(p, blocks, "wrap")
    assert K.same_bits(all_got, exp), "streamed against the dense forward reference: " + K.first_diff(all_got, exp)
    rows = S.concat_rows(blocks)
    with Renderer(hip_lib, options=S.LOOP_DYN) as f:
        p.install(f)
        twin = np.concatenate([f.fill_buffer(p.n_rows, a, min(a + 4800, S.WRAP_FRAMES), [r[a:a + 4800] for r in rows]) for a in range(0, S.WRAP_FRAMES, 4800)], axis=1)
    assert K.same_bits(all_got, twin), "streamed against fr_fill_buffer: " + K.first_diff(all_got, twin)
    assert not S.condition_message(p, all_got)


def test_sparkle_semantics(hip_lib, oracle_lib):
    p = S.case("flanger_8")
    blocks = S.blocks_of(p, [(0, S.FRAMES)], seed=43)
    n, n_dense, n_oracle = stream_and_compare(hip_lib, oracle_lib, p, blocks, "sparkle", semantics="sparkle")
    assert n == n_dense == S.FRAMES and n_oracle == p.oracle


@pytest.mark.parametrize("name", S.STORE_CASES)
def test_store_forms_with_an_edit(hip_lib, name):
    """FR_STREAM_STORE=1: the stream survives an edit of the feedback gain between two blocks (it re-plans and relaunches); every
    block before and after equals the fr_fill_buffer twin given the same edit, and differs from the unedited run after it."""
    p = S.case(name)
    blocks = S.blocks_of(p, [(0, 600)], seed=37)
    edit = 9
    got, first, last = S.stream_blocks(hip_lib, p, blocks, options=dict(p.options, FR_STREAM_STORE="1"), edit_before=edit)
    S.check_stream_object(first, p, store=True)
    S.check_stream_object(last, p, store=True)
    assert last["store"]["on"] is True, last
    twin = S.fill_blocks(hip_lib, p, blocks, edit_before=edit)
    assert S.compare_blocks(got, twin, blocks, f"{name}, store form with an edit, streamed against fr_fill_buffer") == 600
    plain = S.fill_blocks(hip_lib, p, blocks)
    at = sum(T for _, T, _ in blocks[:edit])
    a, b = np.concatenate(got, axis=1), np.concatenate(plain, axis=1)
    assert K.same_bits(a[:, :at], b[:, :at]) and not K.same_bits(a[:, at:], b[:, at:])
    assert not S.condition_message(p, a)
