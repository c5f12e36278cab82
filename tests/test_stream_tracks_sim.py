"""FR_STREAM_TRACKS on the CPU, through the engine's own host code in the host-logic simulator (tests/sim_tools.py) and the oracle.
The simulator has no run-time compiler and no resident launch, so its plans never hold a track bank and no block is ever streamed:
what the rule makes of a track bank is tests/test_stream_tracks_host.py's, what the two track kernels compute -- and that
fr_stream_block_dense equals fr_stream_block_rows on a stream without tracks -- tests/test_hip_stream_tracks.py's.

Covered here: the option's plumbing and strictness; fr_plan_json of plans without a track bank -- unchanged with the option unset
or 0, and with 1 unchanged apart from the new key; fr_stream_block_dense's argument checks and its answer on the simulator, which
is fr_stream_block_rows'; and, before anything runs on a GPU, the conditions on the inputs of every GPU case, proven with
bank_reference.render_track_bank -- re-pinned here to the oracle bit for bit at P = 8 on a hostile block -- and the oracle: every
expected row of a non-hostile voice is at least 95 % finite and louder than 0.01 somewhere over the blocks the GPU test streams,
and consecutive blocks' matrices differ in every row (a stale read of the staging would not pass)."""
import numpy as np
import pytest

import sim_tools
import stream_cases as K
import stream_fx_cases as FX
import stream_tracks_cases as T
import track_rows as TR
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, RenderError, Renderer

STREAM_KEYS = ("FR_LOOP_DYN", "FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN",
               "FR_STREAM_HISTORY", "FR_STREAM_EFFECTS", "FR_STREAM_STORE", "FR_STREAM_TAPS", "FR_STREAM_SWEEP", "FR_STREAM_LEAVES", "FR_STREAM_TRACKS", "FR_LOOP_TILES",
               "FR_STAGE_JIT", "FR_TRACK_HISTORY")


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in STREAM_KEYS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_option_plumbing(sim, clean_env):
    assert sim.has_stream_dense
    with Renderer(sim) as r:
        assert "FR_STREAM_TRACKS" not in r.options()
    for v in ("0", "1"):
        with Renderer(sim, options={"FR_STREAM_TRACKS": v}) as r:
            assert r.options()["FR_STREAM_TRACKS"] == {"value": v, "source": "option"}
    clean_env.setenv("FR_STREAM_TRACKS", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_STREAM_TRACKS"] == {"value": "1", "source": "env"}
    with Renderer(sim, options={"FR_STREAM_TRACKS": "0"}) as r:      # the option beats the environment
        assert r.options()["FR_STREAM_TRACKS"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_STREAM_TRACKS", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_STREAM_TRACKS": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_STREAM_TRACKS", bad)
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


def test_inert_without_its_two_options(sim):
    """FR_STREAM_TRACKS=1 alone: no "stream" object, as without it; with FR_STREAM_PROGRAMS but not FR_STREAM_LEAVES the key is
    there and says that nothing is staged."""
    tree = K.comb_tree(2, 128, 100)
    with Renderer(sim, options={"FR_STREAM_TRACKS": "1"}) as r:
        synth.install(r, tree)
        r.fill_buffer(2, 0, 16, [np.arange(16, dtype=np.float32)])
        assert "stream" not in r.plan()
    with Renderer(sim, options=dict(K.OPTION, FR_STREAM_TRACKS="1")) as r:
        synth.install(r, tree)
        r.fill_buffer(2, 0, 16, [np.arange(16, dtype=np.float32)])
        s = r.plan()["stream"]
        assert s["servable"] is True and s["tracks"] == {"first_slot": 0, "rows": 0, "limit": T.LIMIT} and "leaf_banks" not in s


NO_TRACK_BANK = [
    ("template_bank_with_envelope", lambda: synth.effects_tree(2, 128, taps=0), 2, 1, K.OPTION),
    ("voiceless_echo", lambda: FX.echo_tree(100), 1, 2, FX.INPUTS),
    ("general_voice", lambda: synth.additive_tree(2, 96), 2, 1, dict(K.OPTION, FR_STREAM_GENERAL="1")),
]


@pytest.mark.parametrize("name,build,n_rows,n_in,options", NO_TRACK_BANK, ids=[c[0] for c in NO_TRACK_BANK])
def test_plans_without_a_track_bank_are_unchanged(sim, name, build, n_rows, n_in, options):
    """fr_plan_json with the option unset and 0: the same, key for key; with 1 the stream object gains "tracks" with 0 rows and
    everything else -- servable, the kernel, the reason -- stays."""
    tree = build()
    rows = [np.arange(16, dtype=np.float32)] * n_in
    plans = {}
    for key, extra in (("unset", {}), ("0", {"FR_STREAM_TRACKS": "0"}), ("1", {"FR_STREAM_TRACKS": "1"})):
        with Renderer(sim, options=dict(options, FR_STAGE_JIT="0", FR_STREAM_LEAVES="1", **extra)) as r:
            synth.install(r, tree)
            r.fill_buffer(n_rows, 0, 16, rows)
            plans[key] = {k: v for k, v in r.plan().items() if k not in ("build_ms", "lower_ms", "jit_compile_ms")}
    assert plans["unset"]["stream"]["servable"] is True, plans["unset"]["stream"]
    assert "tracks" not in plans["unset"]["stream"]
    assert plans["unset"] == plans["0"]
    on = dict(plans["1"])
    stream = dict(on.pop("stream"))
    assert stream.pop("tracks") == {"first_slot": 0, "rows": 0, "limit": T.LIMIT}
    off = dict(plans["unset"])
    assert stream == off.pop("stream") and on == off


def test_dense_blocks_on_the_simulator(sim):
    """fr_stream_block_dense checks its arguments as fr_stream_block_rows does, and on the simulator -- no resident launch --
    answers a block with the status and the sentence of fr_stream_block_rows fed the same rows."""
    tree = synth.effects_tree(2, 128, taps=0)
    m = np.stack([synth.time_ramp(0, 8)])
    answers = []
    for dense in (True, False):
        with Renderer(sim, options=K.OPTION) as r:
            synth.install(r, tree)
            with pytest.raises(RenderError) as ei:                      # no stream is open
                r.stream_block_dense(0, m) if dense else r.stream_block_rows(0, list(m))
            assert ei.value.status == FR_ERR_INVALID_ARG
            r.stream_begin(2)
            with pytest.raises(RenderError) as ei:                      # 65 frames
                r.stream_block_dense(0, np.zeros((1, 65), np.float32)) if dense else r.stream_block_rows(0, [np.zeros(65, np.float32)])
            assert ei.value.status == FR_ERR_INVALID_ARG
            with pytest.raises(RenderError) as ei:
                r.stream_block_dense(0, m) if dense else r.stream_block_rows(0, list(m))
            answers.append((ei.value.status, str(ei.value)))
    assert answers[0] == answers[1], answers


# ---- the conditions on the inputs of the GPU cases ------------------------------------------------------------------------------

def test_render_track_bank_is_the_oracle_s(oracle_lib):
    """The dense reference pinned to the oracle, bit for bit, at P = 8 on one hostile block (tests/test_track_variants.py pins it
    at its own shapes): hostile w, amp and time values at every frame of a 64-frame block, under both a full and a cut slot limit."""
    V, P, Tn = 2, 8, 64
    m = TR.regular_rows(V, P, 0, Tn, 7)
    m[0] = TR.hostile_time(0, Tn)
    for k in range(V * P):
        for f in range(Tn):
            if (k + f) % 3 == 0:
                m[1 + 2 * k, f] = TR.HOSTILE_W[(k + 3 * f) % len(TR.HOSTILE_W)]
                m[2 + 2 * k, f] = TR.HOSTILE_AMP[(5 * k + f) % len(TR.HOSTILE_AMP)]
    tree = synth.track_tree(V, P)
    for n_slots in (V, 1):                                              # 2 x 64 = 128 vectors: every row lives; 1 x 64: rows 0..63
        with Renderer(oracle_lib) as o:
            synth.install(o, tree)
            got = o.fill_buffer(n_slots, 0, Tn, list(m))
        exp = TR.expected(V, P, m, n_slots * Tn)[:n_slots]
        assert K.same_bits(got, exp), K.first_diff(got, exp)
    assert np.isnan(exp).any() and np.isfinite(exp).any()


DENSE = [c for c in T.CASES if c.dense]


@pytest.mark.parametrize("c", DENSE, ids=[c.name for c in DENSE])
def test_expected_rows_meet_the_conditions(c):
    """Over the blocks the GPU test streams (the M-voice cases with M = 4): every non-hostile voice's expected row is at least
    95 % finite and louder than 0.01 somewhere; consecutive matrices differ in every row."""
    blocks = T.blocks_of(c, T.SIM_M, [(0, c.frames)])
    assert sum(b[1] for b in blocks) == c.frames and max(b[1] for b in blocks) == 64 and min(b[1] for b in blocks) == 1
    exp = np.concatenate(T.expected_dense(c, T.SIM_M, blocks), axis=1)
    assert exp.shape == (c.n_rows(T.SIM_M), c.frames)
    msg = T.condition_message(c.name, exp, skip=c.exempt)
    assert not msg, msg
    if c.hostile:
        assert not np.isfinite(exp).all()
    msg = T.rows_differ_message(c.name, blocks)
    assert not msg, msg


@pytest.mark.parametrize("name", ["trk_am", "trk_env_bus"])
def test_expected_rows_of_the_oracle_cases(oracle_lib, name):
    """The two cases whose rows are more than a track bank, on the oracle; the store case's edit must be audible."""
    c = T.case(name)
    blocks = T.blocks_of(c, 0, [(0, 600)], seed=37)
    exp = np.concatenate(T.fill_blocks(oracle_lib, c, 0, blocks, csr=True), axis=1)
    assert not T.condition_message(name, exp)
    assert not T.rows_differ_message(name, blocks)
    if name == "trk_am":
        assert any(b[3] is not None and len(b[3][1]) == 0 for b in blocks) and any(b[3] is not None and 0 < len(b[3][1]) < b[1] for b in blocks)
    else:
        tree = c.build()
        a = np.concatenate(T.fill_blocks(oracle_lib, c, 0, blocks, tree=tree, edit_before=9, csr=True), axis=1)
        at = sum(b[1] for b in blocks[:9])
        assert K.same_bits(a[:, :at], exp[:, :at]) and not K.same_bits(a[:, at:], exp[:, at:])
        assert not T.condition_message("trk_env_bus edited", a)


def test_the_other_sequences_and_the_limits(oracle_lib):
    """The short blocks and the seeks meet the conditions; the unprimed case's first limit falls between a w and an amp slot; the
    short case's matrix ends between a w and an amp slot; the dense reference under those limits is the oracle's on a prefix."""
    for name in ("trk_128", "trk_chunks"):
        c = T.case(name)
        blocks = T.short_blocks_of(c)
        assert not T.condition_message(name, np.concatenate(T.expected_dense(c, 0, blocks), axis=1))
    c = T.case("trk_chunks")
    blocks = T.blocks_of(c, 0, [(0, 300), (9000, 200), (2500, 200)], seed=31)
    assert not T.condition_message("trk_chunks seeks", np.concatenate(T.expected_dense(c, 0, blocks), axis=1))
    assert not T.rows_differ_message("trk_chunks seeks", blocks)
    u = T.case("trk_unprimed")
    assert u.n_rows() * 64 == u.first + 2 * 63 + 1                      # the amp slot of partial 63 of voice 0
    s = T.case("trk_short")
    assert (s.short - s.first) % 2 == 1 and s.short < s.n_in()
    for c in (u, s, T.case("trk_hostile")):
        blocks = T.blocks_of(c, 0, [(0, 200)])
        exp = T.fill_blocks(oracle_lib, c, 0, blocks, csr=True)
        assert T.compare_blocks(T.expected_dense(c, 0, blocks), exp, blocks, f"{c.name}: render_track_bank against the oracle") == 200
