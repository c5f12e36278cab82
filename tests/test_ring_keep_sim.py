"""FR_RING_KEEP on the CPU: the engine's own host code in the host-logic simulator (tests/sim_tools.py).  Every sequence of
tests/ring_keep_cases.py is rendered three ways -- the oracle, the option off, the option on -- and all three agree bit for
bit on every call; what the call after an edit launches (voices, programs, frames) is compared with counts derived from
the graphs' structure.  The kernels themselves: tests/test_hip_ring_keep.py."""
import numpy as np
import pytest

import ring_keep_cases as K
import sim_tools
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INPUT_TOO_LONG, FR_ERR_INVALID_ARG, RenderError, Renderer


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_effects_chain_edits(sim, oracle_lib, clean_env):
    K.run_chain_sequence(sim, oracle_lib)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("d", [100, 1])
def test_comb_loops_are_not_replayed_for_edits_outside_them(sim, oracle_lib, clean_env, d):
    """Oracle, option off and option on on every call, the edits included.  The oracle's recursion costs frame / d evaluations
    of a 64-partial voice per frame, so this sequence is short: idx passes the tap's 250-frame look-back but the rings (32768
    frames in a feedback plan) do not wrap; test_comb_loops_at_frame_40000 is the long one."""
    if d == 100:
        K.run_comb_sequence(sim, oracle_lib, d, reach=2500, first=(100, 150, 250), step=400, after=(60, 40))
    else:
        K.run_comb_sequence(sim, oracle_lib, d, reach=500, first=(100, 150, 250), step=100, after=(60, 40))


@pytest.mark.timeout(900)
@pytest.mark.parametrize("d", [100, 1])
def test_comb_loops_at_frame_40000(sim, clean_env, d):
    """The same edits after 40 000 frames, the rings wrapped: option off (a full replay from 0 after every edit) against option
    on, every call.  Beyond what the oracle can follow."""
    K.run_comb_sequence(sim, None, d)


def test_merged_loop(sim, oracle_lib, clean_env):
    K.run_merged_loop(sim, oracle_lib)


@pytest.mark.parametrize("seed0", range(0, 200, 50))
def test_random_edits_between_calls(sim, oracle_lib, clean_env, seed0):
    assert K.run_random_edits(sim, oracle_lib, range(seed0, seed0 + 50)) == 0     # no seed may be passed over


@pytest.mark.timeout(900)
def test_feedback_graphs_edited_during_playback(sim, oracle_lib, clean_env):
    done, off, on = K.run_random_feedback_edits(sim, oracle_lib, range(0, 400))
    assert done >= 200 and on == off and 10 * off <= done, (done, off, on)


@pytest.mark.parametrize("grow", [False, True])
@pytest.mark.parametrize("arrangement", sorted(K.MOVE_ARRANGEMENTS))
@pytest.mark.parametrize("rings", [1, 3, 64])
def test_ring_move_through_the_engine(sim, oracle_lib, clean_env, rings, arrangement, grow):
    """(700 rings: tests/test_hip_ring_keep.py.)"""
    K.run_moves(sim, oracle_lib, rings, arrangement, grow)


# ---- the option -------------------------------------------------------------------------------------------------------

def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_RING_KEEP" not in r.options()
    with Renderer(sim, options={"FR_RING_KEEP": "1"}) as r:
        assert r.options()["FR_RING_KEEP"] == {"value": "1", "source": "option"}
    clean_env.setenv("FR_RING_KEEP", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_RING_KEEP"] == {"value": "1", "source": "env"}
    with Renderer(sim, options={"FR_RING_KEEP": "0"}) as r:          # the option beats the environment
        assert r.options()["FR_RING_KEEP"] == {"value": "0", "source": "option"}
        synth.install(r, synth.effects_tree(2, 8, taps=2, base_delay=20.0))
        r.fill_buffer(2, 0, 64, [synth.time_ramp(0, 64)])
        assert r.plan()["ring_keep"] is False
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_RING_KEEP", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_RING_KEEP": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_RING_KEEP", bad)
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


def test_inert_reasons(sim, clean_env):
    tree = synth.effects_tree(2, 64, taps=2, base_delay=20.0)
    with Renderer(sim, options=K.OPT, history_frames=4096) as r:
        synth.install(r, tree)
        r.fill_buffer(2, 0, 64, [synth.time_ramp(0, 64)])
        p = r.plan()
        assert p["ring_keep"] is True and p["rings"] > 0 and p["ring_state"]["inert"] == "bounded input history", p["ring_state"]
    with Renderer(sim, options=K.OPT) as r:           # rank 0 of 2 under partial-block sharding; the peer's sums arrive as zeros
        def sendrecv(peer, send, recv):
            if recv is not None:
                recv[:] = 0
        r.set_shard(0, 2, mode="partials", sendrecv=sendrecv)
        synth.install(r, tree)
        r.fill_buffer(2, 0, 64, [synth.time_ramp(0, 64)])
        p = r.plan()
        assert p["rings"] > 0 and p["ring_state"]["inert"] == "partial-block sharding", p["ring_state"]
        assert p["ring_state"]["kept"] == 0 and p["ring_state"]["rebuilt"] == p["rings"], p["ring_state"]


def test_inert_under_a_track_window_plan(sim, oracle_lib, clean_env):
    """A track (an envelope row) read by a program that feeds a delay line: the track ring is state of its own, the option
    does nothing and says so; bits as the oracle's."""
    from libfriendship_amd.synth import C, IN, K_DELAY, K_MUL, K_SUM2
    V, P, FIRST = 2, 64, 1
    g = synth.GraphArrays()
    p = synth.voice_params(V, P, 0x5EED0002)
    x = synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P))
    y = g.nodes(K_MUL, V)
    g.edge(0, y, FIRST + np.arange(V, dtype=np.uint32), 0)
    g.edge(x, y, 0, 1)
    out = g.binop(K_SUM2, y, g.binop(K_MUL, C(np.float32(0.5)), g.binop(K_DELAY, y, C(np.float32(10.0)), V), V), V)
    g.edge(out, 0, 0, np.arange(V, dtype=np.uint32))
    tree = g.finish(V)
    rng = np.random.default_rng(5)
    with Renderer(sim, options=dict(K.OPT, FR_TRACK_HISTORY="4800")) as r, Renderer(oracle_lib) as ref:
        r.set_track_inputs(FIRST)
        synth.install(r, tree)
        synth.install(ref, tree)
        idx = 0
        for T in (64, 200, 100):
            m = np.zeros((FIRST + V, T), np.float32)
            m[0] = synth.time_ramp(idx, idx + T)
            m[FIRST:] = rng.normal(size=(V, T)).astype(np.float32)
            assert K.same_bits(r.fill_buffer_dense(V, idx, idx + T, m), ref.fill_buffer_dense(V, idx, idx + T, m))
            idx += T
        pl = r.plan()
        assert pl["track_window_slots"] >= 1 and pl["rings"] > 0, pl
        assert pl["ring_keep"] is True and pl["ring_state"]["inert"] == "track history", pl["ring_state"]


def test_a_call_that_fails_after_the_commit_leaves_nothing_kept(sim, oracle_lib, clean_env):
    """Rank 0 of a voice-sharded job that gathers every row: the gather follows the launches, so a transport that fails there
    fails the call after its inputs were committed and its rings written.  The retry finds nothing marked kept -- everything
    is rebuilt -- and renders the bits of the renderer without the option and (rank 0's rows) of the oracle."""
    ch = K.Chains(4, 64, 2, 50.0)
    state = {"fail": False}

    def sendrecv(peer, send, recv):
        if state["fail"]:
            raise RuntimeError("transport down")
        if recv is not None:
            recv[:] = 0
    t = K.Trio(sim, None, lambda r: synth.install(r, ch.tree))
    ref = Renderer(oracle_lib)
    synth.install(ref, ch.tree)
    try:
        for r in (t.off, t.on):
            r.set_shard(0, 2, mode="voices", gather=True, sendrecv=sendrecv)
        lo, hi = t.on.shard_rows(4)

        def call(T):
            i = t.idx
            off, on = t.call(4, T)
            exp = ref.fill_buffer(4, i, i + T, [synth.time_ramp(i, i + T)])
            return off, on, exp
        for T in (200, 300):
            off, on, exp = call(T)
        assert on["ring_state"]["kept"] == on["rings"] > 0, on["ring_state"]
        state["fail"] = True
        for r in (t.off, t.on):
            with pytest.raises(RenderError):
                r.fill_buffer(4, t.idx, t.idx + 100, [synth.time_ramp(t.idx, t.idx + 100)])
        state["fail"] = False
        i = t.idx
        a = t.off.fill_buffer(4, i, i + 100, [synth.time_ramp(i, i + 100)])
        b = t.on.fill_buffer(4, i, i + 100, [synth.time_ramp(i, i + 100)])
        exp = ref.fill_buffer(4, i, i + 100, [synth.time_ramp(i, i + 100)])
        st = t.on.plan()["ring_state"]
        assert st["kept"] == 0 and st["rebuilt"] == t.on.plan()["rings"] and st["inert"] == "", st
        assert K.same_bits(a, b) and K.same_bits(b[lo:hi], exp[lo:hi])
        t.idx = i + 100
        off, on = t.call(4, 150)
        assert on["ring_state"]["kept"] == on["rings"] and on["ring_state"]["rebuilt"] == 0, on["ring_state"]
    finally:
        ref.close()
        t.close()


def test_a_refused_call_keeps_the_table(sim, oracle_lib, clean_env):
    ch = K.Chains(3, 64, 2, 50.0)
    t = K.Trio(sim, oracle_lib, lambda r: synth.install(r, ch.tree))
    try:
        for T in (200, 300):
            t.call(3, T)
        for r in (t.off, t.on):
            with pytest.raises(RenderError) as ei:
                r.fill_buffer(3, t.idx, t.idx + 10, [synth.time_ramp(0, 11)])     # a row longer than the range
            assert ei.value.status == FR_ERR_INPUT_TOO_LONG
        off, on = t.call(3, 100)
        assert on["ring_state"]["kept"] == on["rings"] and on["ring_state"]["rebuilt"] == 0, on["ring_state"]
        assert K.launches(on, "repair") == ([], [])
    finally:
        t.close()
