"""FR_STREAM_TRACKS on the MI355X: the two track kernels (bank_stream_track_kernel, bank_stream_track_store_kernel; csrc/kernels.hpp)
and fr_stream_block_dense.

Every case of tests/stream_tracks_cases.py is streamed from frame 0 in blocks of 1..64 frames (1500 frames; the M-voice cases 300)
after one priming dense call, and every streamed sample is compared bit for bit (NaN equal to NaN, +0 unequal to -0)
  (i)   with fr_fill_buffer_dense of the same blocks on a second HIP renderer without a stream option: the hipRTC-generated jit_bank
        kernel with tracks, an independent evaluator of the same leaves;
  (ii)  with bank_reference.render_track_bank on every frame, under the reference's slot limit (the synth.track_tree cases and
        trk_carry; not the two cases whose rows are more than a track bank: trk_am, trk_env_bus);
  (iii) with the C++ oracle on a prefix; for the M-voice cases (M = stream.max_workgroups, 256 on a whole MI355X) the oracle renders
        a patch that holds only voices 0 and M - 1, with the slots they have in the whole patch.
Further: blocks of 64, 1 and 37 frames from frame 0; jumps as seeks; the Sparkle semantics on the hostile case; the store form
across an edit of one template partial's amplitude on trk_env_bus; fr_stream_block_dense against fr_stream_block_rows on streams
without tracks; the "stream" object; with the option unset and 0 every case is refused with the parent's sentence; a track history
is refused with its sentence.

Renderers compile in the call (FR_CONFIG_SYNC_COMPILE, capi.Renderer's default).  tests/test_stream_tracks_sim.py has proven on the
CPU that every expected row but the hostile voices' is at least 95 % finite and audible and that consecutive matrices differ in
every row.  One streaming renderer at a time; the twin renders after the stream is closed."""
import numpy as np
import pytest

import stream_cases as K
import stream_fx_cases as FX
import stream_tracks_cases as T
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_UNSUPPORTED, RenderError, Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_LOOP_DYN", "FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN",
              "FR_STREAM_HISTORY", "FR_STREAM_EFFECTS", "FR_STREAM_STORE", "FR_STREAM_TAPS", "FR_STREAM_SWEEP", "FR_STREAM_LEAVES", "FR_STREAM_TRACKS", "FR_LOOP_TILES",
              "FR_STREAM_IDLE_MS", "FR_RING_KEEP", "FR_STAGE_JIT", "FR_JIT", "FR_TRACK_HISTORY"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def max_wgs(hip_lib):
    """stream.max_workgroups of this device (256 on a whole MI355X)."""
    with Renderer(hip_lib, options=dict(T.OPTION, FR_STREAM_BANKS="1")) as r:
        r.set_track_inputs(1)
        synth.install(r, T.track_tree(1, 128))
        r.fill_buffer_dense(1, 0, 8, np.zeros((257, 8), np.float32))
        return int(r.plan()["stream"]["max_workgroups"])


def stream_and_compare(hip_lib, oracle_lib, c, M, blocks, key, semantics="reference", oracle=True):
    tree = c.build(M)
    got, first, last = T.stream_blocks(hip_lib, c, M, blocks, semantics=semantics, tree=tree)
    T.check_stream_object(first, c, M)
    T.check_stream_object(last, c, M)
    twin = T.fill_blocks(hip_lib, c, M, blocks, semantics=semantics, tree=tree)
    n = T.compare_blocks(got, twin, blocks, f"{c.name} [{key}], streamed against fr_fill_buffer_dense (the generated kernel)")
    n_dense = 0
    if c.dense and semantics == "reference":
        n_dense = T.compare_blocks(got, T.expected_dense(c, M, blocks), blocks, f"{c.name} [{key}], streamed against render_track_bank")
    n_oracle = 0
    if oracle:
        sample = c.sample(M) if c.sample else None
        exp = T.fill_blocks(oracle_lib, c, M, blocks, semantics=semantics, tree=c.build(M, sample) if sample else tree, n_rows=len(sample) if sample else None,
                            upto=c.oracle, csr=True)
        n_oracle = T.compare_blocks(got, exp, blocks, f"{c.name} [{key}], streamed against the oracle", rows=sample)
    assert not T.condition_message(c.name, np.concatenate(got, axis=1), skip=c.exempt)
    print(f"{c.name} [{key}]: {n} frames x {c.n_rows(M)} rows compared with fr_fill_buffer_dense, {n_dense} with render_track_bank, {n_oracle} with the oracle; "
          f"{last['kernel']}; tracks {last['tracks']}")
    return n, n_dense, n_oracle


@pytest.mark.parametrize("c", T.CASES, ids=T.IDS)
def test_every_streamed_sample(hip_lib, oracle_lib, max_wgs, c):
    blocks = T.blocks_of(c, max_wgs, [(0, c.frames)])
    n, n_dense, n_oracle = stream_and_compare(hip_lib, oracle_lib, c, max_wgs, blocks, "main")
    assert n == c.frames and n_dense == (c.frames if c.dense else 0) and n_oracle == min(c.oracle, c.frames)
    if c.name == "trk_cap" and max_wgs == 256:
        assert c.staged(max_wgs) == T.LIMIT


@pytest.mark.parametrize("name", ["trk_128", "trk_chunks"])
def test_short_blocks_from_frame_0(hip_lib, oracle_lib, name):
    c = T.case(name)
    blocks = T.short_blocks_of(c)
    assert [b[1] for b in blocks] == [64, 1, 37]
    assert stream_and_compare(hip_lib, oracle_lib, c, 0, blocks, "short") == (102, 102, 102)


def test_jumps_are_seeks(hip_lib):
    """[(0, 300), (9000, 200), (2500, 200)]: a block that does not continue the previous one retires the launch; the streamed
    blocks equal fr_fill_buffer_dense's, which seeks at the same frames, and the dense reference."""
    c = T.case("trk_chunks")
    blocks = T.blocks_of(c, 0, [(0, 300), (9000, 200), (2500, 200)], seed=31)
    got, first, last = T.stream_blocks(hip_lib, c, 0, blocks)
    T.check_stream_object(last, c)
    assert T.compare_blocks(got, T.fill_blocks(hip_lib, c, 0, blocks), blocks, "trk_chunks, seeks, streamed against fr_fill_buffer_dense") == 700
    assert T.compare_blocks(got, T.expected_dense(c, 0, blocks), blocks, "trk_chunks, seeks, streamed against render_track_bank") == 700


def test_hostile_rows_under_sparkle_semantics(hip_lib, oracle_lib):
    c = T.case("trk_hostile")
    blocks = T.blocks_of(c, 0, [(0, c.frames)], seed=43)
    assert stream_and_compare(hip_lib, oracle_lib, c, 0, blocks, "sparkle", semantics="sparkle") == (c.frames, 0, c.frames)


def test_store_form_with_an_edit(hip_lib):
    """FR_STREAM_STORE=1 on trk_env_bus: the stream stores its time row (never its tracks) and survives an edit of one template
    amplitude between two blocks (it re-plans and relaunches); every block before and after equals the fr_fill_buffer_dense twin given the same edit, and
    differs from the unedited run after it."""
    c = T.case("trk_env_bus")
    blocks = T.blocks_of(c, 0, [(0, 600)], seed=37)
    tree, edit = c.build(), 9
    got, first, last = T.stream_blocks(hip_lib, c, 0, blocks, options=dict(c.options, FR_STREAM_STORE="1"), edit_before=edit, tree=tree)
    T.check_stream_object(first, c, store=True)
    T.check_stream_object(last, c, store=True)
    assert last["store"]["on"] is True, last
    twin = T.fill_blocks(hip_lib, c, 0, blocks, tree=tree, edit_before=edit)
    assert T.compare_blocks(got, twin, blocks, "trk_env_bus, store form with an edit, streamed against fr_fill_buffer_dense") == 600
    plain = T.fill_blocks(hip_lib, c, 0, blocks, tree=tree)
    at = sum(b[1] for b in blocks[:edit])
    a, b = np.concatenate(got, axis=1), np.concatenate(plain, axis=1)
    assert K.same_bits(a[:, :at], b[:, :at]) and not K.same_bits(a[:, at:], b[:, at:])
    assert not T.condition_message("trk_env_bus edited", a)


NO_TRACKS = [
    ("template_bank_with_envelope", lambda: synth.effects_tree(2, 128, taps=0), 2, 1, K.OPTION),
    ("echo_on_a_control_row", lambda: FX.echo_tree(100), 1, 2, FX.INPUTS),
]


@pytest.mark.parametrize("name,build,n_rows,n_in,options", NO_TRACKS, ids=[c[0] for c in NO_TRACKS])
def test_dense_blocks_equal_row_blocks_without_tracks(hip_lib, name, build, n_rows, n_in, options):
    """On a stream without tracks fr_stream_block_dense is fr_stream_block_rows fed the same full-length rows, bit for bit (the
    simulator has no resident launch, so this stands here)."""
    tree = build()
    rng = np.random.default_rng(5)
    blocks = [(idx, np.array(t, np.float32)) for idx, t in K.finite_block_rows(rng, [(0, 400)])]
    mats = [np.stack([t] + [rng.uniform(-1, 1, len(t)).astype(np.float32) for _ in range(n_in - 1)]) for _, t in blocks]
    outs = []
    for dense in (True, False):
        with Renderer(hip_lib, options=dict(options, **T.IDLE)) as r:
            synth.install(r, tree)
            r.stream_begin(n_rows)
            outs.append([r.stream_block_dense(idx, m) if dense else r.stream_block_rows(idx, list(m)) for (idx, _), m in zip(blocks, mats)])
            assert "track" not in r.plan()["stream"]["kernel"]
            r.stream_end()
    for k, (a, b) in enumerate(zip(*outs)):
        assert K.same_bits(a, b), f"{name}: block {k}: " + K.first_diff(a, b)
    assert np.nanmax(np.abs(np.concatenate(outs[0], axis=1))) > T.LOUD


def test_stream_object(hip_lib):
    """servable, kernel, tracks, leaf_banks and input_slots before any block is streamed."""
    for name in ("trk_128", "trk_am", "trk_env_bus"):
        c = T.case(name)
        with Renderer(hip_lib, options=c.options) as r:
            r.set_track_inputs(c.first)
            synth.install(r, c.build())
            r.fill_buffer_dense(c.n_rows(), 0, 8, T.blocks_of(c, 0, [(0, 8)])[0][2][:, :8].copy())
            plan = r.plan()
        s = plan["stream"]
        T.check_stream_object(s, c)
        assert sum(1 for b in plan["banks"] if b["jit"]) == 1 and len(plan["banks"]) == c.banks, plan["banks"]
        if name == "trk_env_bus":
            assert sorted(b["to_ring"] for b in s["banks"]) == [False, True] and s["bus_programs"] == 1, s


@pytest.mark.parametrize("c", T.CASES, ids=T.IDS)
def test_refused_with_the_option_off(hip_lib, max_wgs, c):
    """FR_STREAM_TRACKS unset and 0: fr_stream_begin refuses the patch with the parent's sentence."""
    M = min(max_wgs, 2)
    tree, n_rows = c.build(M), c.n_rows(M)
    for tracks in (None, "0"):
        options = {k: v for k, v in c.options.items() if k != "FR_STREAM_TRACKS"}
        if tracks is not None:
            options["FR_STREAM_TRACKS"] = tracks
        with Renderer(hip_lib, options=options) as r:
            r.set_track_inputs(c.first)
            synth.install(r, tree)
            with pytest.raises(RenderError) as ei:
                r.stream_begin(n_rows)
            assert ei.value.status == FR_ERR_UNSUPPORTED and T.OLD_REASON in str(ei.value), str(ei.value)
            s = r.plan()["stream"]
            assert s["servable"] is False and s["reason"] == T.OLD_REASON and s["kernel"] == "" and "tracks" not in s, s


def test_a_track_history_is_refused(hip_lib):
    c = T.case("trk_128")
    with Renderer(hip_lib, options=dict(c.options, FR_TRACK_HISTORY="64")) as r:
        r.set_track_inputs(c.first)
        synth.install(r, c.build())
        with pytest.raises(RenderError) as ei:
            r.stream_begin(2)
        assert ei.value.status == FR_ERR_UNSUPPORTED and T.HISTORY_REASON in str(ei.value), str(ei.value)
