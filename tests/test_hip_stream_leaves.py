"""FR_STREAM_LEAVES on the MI355X: the two leaf kernels (bank_stream_leaf_kernel, bank_stream_leaf_store_kernel; csrc/kernels.hpp).

Every case of tests/stream_leaves_cases.py is streamed from frame 0 in blocks of 1..64 frames (1500 frames; the two M-voice cases
300), and every streamed sample is compared bit for bit (NaN equal to NaN, +0 unequal to -0)
  * with fr_fill_buffer of the same blocks on a second HIP renderer without a stream option: the hipRTC-generated jit_bank kernel,
    an independent evaluator of the same leaves;
  * with the C++ oracle on the case's prefix; for the M-voice cases (M = stream.max_workgroups, 256 on a whole MI355X) the oracle
    renders a patch that holds only the two sampled voices, with the same parameters.
Further: blocks of 64, 1 and 37 frames from frame 0; jumps as seeks on the leaf that reads a control row; the Sparkle semantics on
the hostile time row; the store form with an edit of one amplitude between two blocks -- what follows must equal the
fr_fill_buffer twin given the same edit --; the "stream" object; with the feature off fr_stream_begin refuses every one of these
patches with the sentence it has always had; and each shape that stays refused is refused with its own sentence.

Renderers compile in the call (FR_CONFIG_SYNC_COMPILE, capi.Renderer's default), so a plan has its compiled banks from the first
call.  tests/test_stream_leaves_sim.py has proven on the CPU that every expected row but the hostile case's is at least 95 %
finite and audible.  One streaming renderer at a time; the twin renders after the stream is closed."""
import numpy as np
import pytest

import stream_cases as K
import stream_leaves_cases as L
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_UNSUPPORTED, RenderError, Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_LOOP_DYN", "FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN",
              "FR_STREAM_HISTORY", "FR_STREAM_EFFECTS", "FR_STREAM_STORE", "FR_STREAM_TAPS", "FR_STREAM_SWEEP", "FR_STREAM_LEAVES", "FR_LOOP_TILES", "FR_STREAM_IDLE_MS",
              "FR_RING_KEEP", "FR_STAGE_JIT", "FR_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def max_wgs(hip_lib):
    """stream.max_workgroups of this device (256 on a whole MI355X)."""
    with Renderer(hip_lib, options=dict(L.OPTION, FR_STREAM_BANKS="1")) as r:
        synth.install(r, L.tri_tree(1, 128))
        r.fill_buffer(1, 0, 8, [np.arange(8, dtype=np.float32)])
        return int(r.plan()["stream"]["max_workgroups"])


def stream_and_compare(hip_lib, oracle_lib, c, M, blocks, key, semantics="reference", oracle=True):
    tree, n_rows = c.build(M), c.n_rows(M)
    got, first, last = L.stream_blocks(hip_lib, tree, n_rows, blocks, c.options, semantics=semantics)
    L.check_stream_object(first, c, M)
    L.check_stream_object(last, c, M)
    twin = L.fill_blocks(hip_lib, tree, n_rows, blocks, semantics=semantics)
    n = L.compare_blocks(got, twin, blocks, f"{c.name} [{key}], streamed against fr_fill_buffer (the compiled kernel)")
    n_oracle = 0
    if oracle:
        sample = c.sample(M) if c.sample else None
        exp = L.fill_blocks(oracle_lib, c.oracle_build(M) if sample else tree, len(sample) if sample else n_rows, blocks, semantics=semantics, upto=c.oracle)
        n_oracle = L.compare_blocks(got, exp, blocks, f"{c.name} [{key}], streamed against the oracle", rows=sample)
    all_got = np.concatenate(got, axis=1)
    if not c.hostile:
        assert not L.condition_message(c.name, all_got)
    print(f"{c.name} [{key}]: {n} frames x {n_rows} rows compared with fr_fill_buffer, {n_oracle} with the oracle; {last['kernel']}; leaf_banks {last['leaf_banks']}")
    return n, n_oracle


@pytest.mark.parametrize("c", L.CASES, ids=L.IDS)
def test_every_streamed_sample(hip_lib, oracle_lib, max_wgs, c):
    blocks = L.blocks_of(c, [(0, c.frames)])
    n, n_oracle = stream_and_compare(hip_lib, oracle_lib, c, max_wgs, blocks, "main")
    assert n == c.frames and n_oracle == min(c.oracle, c.frames)


@pytest.mark.parametrize("name", ["tri_128", "tri_chunks"])
def test_short_blocks_from_frame_0(hip_lib, oracle_lib, name):
    c = L.case(name)
    blocks = L.short_blocks_of(c)
    assert [T for _, T, _ in blocks] == [64, 1, 37]
    assert stream_and_compare(hip_lib, oracle_lib, c, 0, blocks, "short") == (102, 102)


def test_jumps_are_seeks(hip_lib):
    """[(0, 300), (9000, 200), (2500, 200)] on the leaf that reads a control row: a block that does not continue the previous one
    retires the launch; the streamed blocks equal fr_fill_buffer's, which seeks at the same frames."""
    c = L.case("tri_am")
    blocks = L.blocks_of(c, [(0, 300), (9000, 200), (2500, 200)], seed=31)
    tree = c.build()
    got, first, last = L.stream_blocks(hip_lib, tree, 2, blocks, c.options)
    L.check_stream_object(last, c)
    assert L.compare_blocks(got, L.fill_blocks(hip_lib, tree, 2, blocks), blocks, "tri_am, seeks, streamed against fr_fill_buffer") == 700
    assert not L.condition_message("tri_am seeks", np.concatenate(got, axis=1))


def test_hostile_times_under_sparkle_semantics(hip_lib, oracle_lib):
    c = L.case("tri_hostile")
    blocks = L.blocks_of(c, [(0, c.frames)], seed=43)
    assert stream_and_compare(hip_lib, oracle_lib, c, 0, blocks, "sparkle", semantics="sparkle") == (c.frames, c.frames)


def test_store_form_with_an_edit(hip_lib):
    """FR_STREAM_STORE=1 on tri_env_bus: the stream survives an edit of one triangle amplitude between two blocks (it re-plans and
    relaunches with the new parameter table); every block before and after equals the fr_fill_buffer twin given the same edit, and
    differs from the unedited run after it."""
    c = L.case("tri_env_bus")
    blocks = L.blocks_of(c, [(0, 600)], seed=37)
    tree, edit = c.build(), 9
    got, first, last = L.stream_blocks(hip_lib, tree, 1, blocks, dict(c.options, FR_STREAM_STORE="1"), edit_before=edit)
    L.check_stream_object(first, c, store=True)
    L.check_stream_object(last, c, store=True)
    assert last["kernel"] == "bank_stream_leaf_store_kernel" and last["store"]["on"] is True and last["store"]["continued"] is True, last
    twin = L.fill_blocks(hip_lib, tree, 1, blocks, edit_before=edit)
    assert L.compare_blocks(got, twin, blocks, "tri_env_bus, store form with an edit, streamed against fr_fill_buffer") == 600
    plain = L.fill_blocks(hip_lib, tree, 1, blocks)
    at = sum(T for _, T, _ in blocks[:edit])
    a, b = np.concatenate(got, axis=1), np.concatenate(plain, axis=1)
    assert K.same_bits(a[:, :at], b[:, :at]) and not K.same_bits(a[:, at:], b[:, at:])
    assert not L.condition_message("tri_env_bus edited", a)


def test_stream_object(hip_lib):
    """servable, kernel, leaf_banks, input_slots, and the banks of the bus case, before any block is streamed."""
    for name in ("tri_128", "tri_am", "literal_alias", "tri_env_bus"):
        c = L.case(name)
        rows = L.blocks_of(c, [(0, 8)])[0][2]
        with Renderer(hip_lib, options=c.options) as r:
            synth.install(r, c.build())
            r.fill_buffer(c.n_rows(), 0, 8, rows)
            plan = r.plan()
        s = plan["stream"]
        L.check_stream_object(s, c)
        assert sum(1 for b in plan["banks"] if b["jit"]) == len(c.leaf_banks) and len(plan["banks"]) == c.banks, plan["banks"]
        if name == "tri_env_bus":
            assert [b["to_ring"] for b in s["banks"]] == [True, True] and s["bus_programs"] == 1, s
        if name == "tri_am":
            assert s["input_slots"] == [0, 1], s


@pytest.mark.parametrize("c", L.CASES, ids=L.IDS)
def test_refused_with_the_feature_off(hip_lib, max_wgs, c):
    """FR_STREAM_LEAVES unset and 0: fr_stream_begin refuses the patch with the sentence it has always had -- the program path's
    for a plan with programs or several banks, the plain path's for one compiled bank that writes the rows."""
    M = min(max_wgs, 2)                                              # (the answer does not depend on how many voices there are)
    tree, n_rows = c.build(M), c.n_rows(M)
    rows = L.blocks_of(c, [(0, 8)])[0][2]
    for leaves in (None, "0"):
        options = {k: v for k, v in c.options.items() if k != "FR_STREAM_LEAVES"}
        if leaves is not None:
            options["FR_STREAM_LEAVES"] = leaves
        with Renderer(hip_lib, options=options) as r:
            synth.install(r, tree)
            r.fill_buffer(n_rows, 0, 8, rows)
            plan = r.plan()
            assert any(b["jit"] for b in plan["banks"]), plan["banks"]
            s = plan["stream"]
            assert s["servable"] is False and s["reason"] == L.OLD_REASON and s["kernel"] == "" and "leaf_banks" not in s, s
            with pytest.raises(RenderError) as ei:
                r.stream_begin(n_rows)
            assert ei.value.status == FR_ERR_UNSUPPORTED
            assert (L.OLD_REASON if c.banks > 1 else L.OLD_REASON_PLAIN) in str(ei.value), str(ei.value)


@pytest.mark.parametrize("name,build,n_rows,options,tracks,sentence", L.STILL_REFUSED, ids=[r[0] for r in L.STILL_REFUSED])
def test_still_refused_shapes(hip_lib, name, build, n_rows, options, tracks, sentence):
    tree = build()
    with Renderer(hip_lib, options=options) as r:
        if tracks is not None:
            r.set_track_inputs(tracks)
        synth.install(r, tree)
        with pytest.raises(RenderError) as ei:
            r.stream_begin(n_rows)
        assert ei.value.status == FR_ERR_UNSUPPORTED and sentence in str(ei.value), str(ei.value)
        s = r.plan()["stream"]
        assert s["servable"] is False and s["reason"] == sentence and s["kernel"] == "" and s["leaf_banks"] == [], s
