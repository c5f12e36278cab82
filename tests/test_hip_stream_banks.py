"""FR_STREAM_BANKS on the GPU: block streaming of plans of several banks (bank_stream_banks_kernel: the bank table is a launch
argument, every workgroup finds its bank, voice and chunk from it; chunk sums, tickets and programs go by the global voice
number).  A dozen blocks go through fr_stream_block / fr_stream_block_rows; then, after the stream is closed (nothing else
renders while a launch is resident: stream_cases.stream_against_fill_buffer explains), the same calls go through
fr_fill_buffer of a second HIP renderer with every stream option off, and through the oracle.  Every status must be equal
and every sample equal bit for bit, NaN equal to NaN.  The serving rule: tests/test_stream_banks_sim.py; the chunk rule on its
own: tests/test_stream_banks_host.py.

Each test has one streaming renderer at a time.  A block that is not answered ends the stream within the engine's own bounds
(250 ms per block, FR_STREAM_IDLE_MS for the launch)."""
import numpy as np
import pytest

import stream_banks_cases as M
import stream_input_cases as I
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_UNSUPPORTED, FR_OK, RenderError, Renderer, f32_bits
from stream_cases import first_diff, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_IDLE_MS", "FR_RING_KEEP", "FR_TRACK_HISTORY",
              "FR_DELAY_OBSERVED", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def trees():
    return {}


def tree_of(trees, table, name):
    if name not in trees:
        trees[name] = M.case(table, name)[1]()
    return trees[name]


HOSTILE_TIMES = np.array([-1.0, -0.0, 4294967808.0, 1e30, np.nan, -np.inf], np.float32)


def blocks_for(rng, n_in):
    """[(idx, T, rows)], 12 blocks: lengths 64, 1, 17 and 63 mixed; block 5 seeks forwards, block 9 backwards; block 2's time
    row is hostile (negative, above 2^32, NaN: the general leaf path, in every bank), block 3's is short, block 4's empty (it
    continues with the slot's last value); control rows (slots 1 .. n_in - 1) of every kind."""
    lengths = [64, 1, 17, 63, 64, 64, 17, 63, 64, 1, 64, 17]
    out, idx = [], 300
    for k, T in enumerate(lengths):
        if k == 5:
            idx = 9000
        if k == 9:
            idx = 2500
        t = synth.time_ramp(idx, idx + T)
        if k == 2 or k == 10:
            t = t.copy()
            t[rng.integers(T, size=6)] = HOSTILE_TIMES
        if k == 3:
            t = t[:T // 2]
        if k == 4:
            t = t[:0]
        seek = k in (0, 5, 9)
        out.append((idx, T, [t] + [I.control_row(rng, T, 0 if seek else int(rng.integers(6))) for _ in range(1, n_in)]))
        idx += T
    return out


def call(fn):
    try:
        return FR_OK, fn()
    except RenderError as e:
        return e.status, None


def fill_all(lib, tree, n_rows, blocks, semantics="reference"):
    with Renderer(lib, semantics=semantics) as f:
        synth.install(f, tree)
        return [call(lambda: f.fill_buffer(n_rows, idx, idx + T, rows)) for idx, T, rows in blocks]


def compare(got, exp, blocks, what):
    for k, ((idx, T, rows), (st, a), (st_e, b)) in enumerate(zip(blocks, got, exp)):
        assert st == st_e, f"block {k} at frame {idx} (T={T}): status {st} streamed, {st_e} {what}"
        if st == FR_OK:
            assert same_bits(a, b), f"block {k} at frame {idx} (T={T}, {[len(r) for r in rows]} values) {what}: " + first_diff(a, b)


def loud(got):
    return max(float(np.nanmax(np.abs(np.where(np.isfinite(a), a, 0)))) for st, a in got if st == FR_OK)


@pytest.mark.parametrize("name", [c[0] for c in M.SERVABLE])
def test_every_case_every_sample(hip_lib, oracle_lib, trees, name):
    _, _, n_rows, options, banks, per_voice, bus, slots = M.case(M.SERVABLE, name)
    tree = tree_of(trees, M.SERVABLE, name)
    rng = np.random.default_rng(len(name) * 7919)
    blocks = blocks_for(rng, len(slots))
    one_row = len(slots) == 1
    with Renderer(hip_lib, options=M.STREAM_OPTIONS) as s:
        synth.install(s, tree)
        s.stream_begin(n_rows)
        got = []
        for idx, T, rows in blocks:
            if one_row and len(rows[0]) == T:                         # the one-row entry point where the row is whole
                got.append(call(lambda: s.stream_block(idx, rows[0])))
            else:
                got.append(call(lambda: s.stream_block_rows(idx, rows, n_times=T)))
        plan = s.plan()
        s.stream_end()
    st = plan["stream"]
    reported = M.check_stream_object(st, banks, per_voice, bus, slots)
    assert len(reported) >= 2
    if len({p for _, p, _ in banks}) > 1:                              # several sizes: one bank is chunked and one is not
        assert any(b["chunks"] > 1 for b in st["banks"]) and any(b["chunks"] == 1 for b in st["banks"]), st
    assert all(s_ == FR_OK for s_, _ in got), [s_ for s_, _ in got]
    compare(got, fill_all(hip_lib, tree, n_rows, blocks), blocks, "through fr_fill_buffer")
    compare(got, fill_all(oracle_lib, tree, n_rows, blocks), blocks, "on the oracle")
    assert loud(got) > 0.01


@pytest.mark.parametrize("semantics", ["sparkle"])
def test_the_chord_under_sparkle_semantics(hip_lib, oracle_lib, trees, semantics):
    tree = tree_of(trees, M.SERVABLE, "chord_bus_taps")
    blocks = blocks_for(np.random.default_rng(3), 1)
    with Renderer(hip_lib, semantics=semantics, options=M.STREAM_OPTIONS) as s:
        synth.install(s, tree)
        s.stream_begin(2)
        got = [call(lambda: s.stream_block_rows(idx, rows, n_times=T)) for idx, T, rows in blocks]
        assert s.plan()["stream"]["kernel"] == M.NEW_KERNEL
        s.stream_end()
    compare(got, fill_all(oracle_lib, tree, 2, blocks, semantics), blocks, "on the oracle")


def test_an_edit_ends_the_stream_and_the_next_one_renders_the_new_graph(hip_lib, trees):
    """chord_bus with an edit between two blocks: the stream is retired, begun again, and the results still match.  (The
    comparison renderer `f` only ever runs while no resident launch does.)"""
    tree = tree_of(trees, M.SERVABLE, "chord_bus")
    n_rows, V = 2, sum(v for v, _ in M.CHORD)
    e = tree["edges"].copy()
    # the edit: voice 1's gain (a constant of a bus program; the voices stay template voices of their banks)
    import stream_bus_cases as B
    j = int(np.nonzero((e[:, 0] == synth.CONST_HANDLE) & (e[:, 3] == 0) & (e[:, 2] == synth.bits(B.gains(V)[1])))[0][0])
    new = f32_bits(np.float32(0.3))
    rounds = []
    with Renderer(hip_lib, options=M.STREAM_OPTIONS) as s:
        synth.install(s, tree)
        idx = 100
        for rnd in range(2):
            s.stream_begin(n_rows)
            blocks = []
            for T in (64, 17, 64, 63):
                blocks.append((idx, T, [synth.time_ramp(idx, idx + T)]))
                idx += T
            got = [call(lambda: s.stream_block(i, rows[0])) for i, T, rows in blocks]
            assert s.plan()["stream"]["kernel"] == M.NEW_KERNEL
            rounds.append((blocks, got))
            if rnd == 0:
                s.on_del_edge(synth.CONST_HANDLE, int(e[j, 1]), int(e[j, 2]), 0)
                s.on_add_edge(synth.CONST_HANDLE, int(e[j, 1]), new, 0)
                with pytest.raises(RenderError):
                    s.stream_block(idx, synth.time_ramp(idx, idx + 8))    # the edit retired the stream
                idx += 37                                                 # (the next stream starts with a seek)
        s.stream_end()
    with Renderer(hip_lib) as f:
        synth.install(f, tree)
        for rnd, (blocks, got) in enumerate(rounds):
            exp = [call(lambda: f.fill_buffer(n_rows, i, i + T, rows)) for i, T, rows in blocks]
            compare(got, exp, blocks, f"through fr_fill_buffer (round {rnd})")
            if rnd == 0:
                f.on_del_edge(synth.CONST_HANDLE, int(e[j, 1]), int(e[j, 2]), 0)
                f.on_add_edge(synth.CONST_HANDLE, int(e[j, 1]), new, 0)
    a, b = rounds[0][1][0][1], rounds[1][1][0][1]
    assert loud(rounds[0][1]) > 0.01 and not same_bits(a, b)


@pytest.mark.parametrize("name", [c[0] for c in M.REFUSED])
def test_refusals_leave_the_renderer_usable(hip_lib, trees, name):
    _, _, n_rows, n_banks, why = M.case(M.REFUSED, name)
    tree = tree_of(trees, M.REFUSED, name)
    with Renderer(hip_lib, options=M.STREAM_OPTIONS) as r:
        synth.install(r, tree)
        with pytest.raises(RenderError) as ei:
            r.stream_begin(n_rows)
        assert ei.value.status == FR_ERR_UNSUPPORTED and why in str(ei.value), str(ei.value)
        out = r.fill_buffer(n_rows, 0, 16, [synth.time_ramp(0, 16)])
        assert out.shape == (n_rows, 16) and np.abs(out).max() > 0.01
        assert len(r.plan()["banks"]) == n_banks


def test_without_the_option_the_chord_is_refused_as_before(hip_lib, trees):
    tree = tree_of(trees, M.SERVABLE, "chord_bus")
    with Renderer(hip_lib, options=I.STREAM_OPTIONS) as r:
        synth.install(r, tree)
        with pytest.raises(RenderError) as ei:
            r.stream_begin(2)
        assert ei.value.status == FR_ERR_UNSUPPORTED and M.old_reason(3) in str(ei.value), str(ei.value)
        assert r.fill_buffer(2, 0, 32, [synth.time_ramp(0, 32)]).shape == (2, 32)


def test_one_bank_keeps_its_kernel(hip_lib):
    """With every option on, a single-bank plan still runs the kernel it ran before."""
    import stream_bus_cases as B
    import stream_cases as K
    rows = K.block_rows(np.random.default_rng(2), [(50, 300)])
    got, plan = B.stream_against_fill_buffer(hip_lib, B.mixdown_tree(2, 1024, 1), 1, rows, options=M.STREAM_OPTIONS)
    s = plan["stream"]
    assert s["kernel"] == "bank_stream_bus_kernel" and len(s["banks"]) == 1 and s["workgroups"] == 16


@pytest.mark.parametrize("silent", [(1, 128, 0), (2, 256, 1)])
def test_a_silent_voice_in_short_blocks(hip_lib, silent):
    """A bank of one voice of 128 partials (one chunk, one group of 8 partials per wave) next to a bank of two voices of 256 in
    chunks of 128; a full block, a block of one frame and a last block of 37; one voice silent -- the one-chunk voice, then a
    chunked one: its chunk sums are exact zeros, whose sign the kernel finds from the leaves."""
    import stream_cases as K
    V, P, v = silent
    tree = K.silence_voice(M.rows_tree([(1, 128), (2, 256)]), V, P, v)
    row = 0 if P == 128 else 1 + v
    blocks = [(idx, len(t), [t]) for idx, t in K.short_blocks()]
    with Renderer(hip_lib, options=M.STREAM_OPTIONS) as s:
        synth.install(s, tree)
        s.stream_begin(3)
        got = [call(lambda: s.stream_block(idx, rows[0])) for idx, T, rows in blocks]
        st = s.plan()["stream"]
        s.stream_end()
    assert st["servable"] and st["kernel"] == M.NEW_KERNEL and sorted((b["voices"], b["partials"], b["chunks"]) for b in st["banks"]) == [(1, 128, 1), (2, 256, 2)], st
    compare(got, fill_all(hip_lib, tree, 3, blocks), blocks, "through fr_fill_buffer")
    assert [a.shape for _, a in got] == [(3, 64), (3, 1), (3, 37)]
    assert not any(a[row].any() for _, a in got) and loud(got) > 0.01
