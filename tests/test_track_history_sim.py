"""FR_TRACK_HISTORY on the CPU: the engine's own host code in the host-logic simulator (tests/sim_tools.py) against the
oracle, bit for bit.  With the option on, the renderer keeps the last H frames of every track row (fr_set_track_inputs) on
the device, so stage programs, Delays of tracks, template voices timed by a track and pull rows may read tracks too; what
the history cannot serve is refused with FR_ERR_UNSUPPORTED and leaves the renderer as it was.  The oracle gets the same
rows as ordinary inputs.  (No run-time compiler in the simulator: no track voices here; tests/test_hip_track_history.py.)"""
import numpy as np
import pytest

import randgraph
import sim_tools
from kat_replay import same_bits
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, FR_ERR_UNSUPPORTED, RenderError, Renderer, f32_bits
from libfriendship_amd.synth import IN, K_DELAY, K_MUL, K_SUM2, C

H = 4800
CALLS = (1, 64, 700, 4800)
V, P = 3, 8
FIRST = 1          # slot 0: time; slots FIRST ..: tracks


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_DELAY_OBSERVED_MAX"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def opts(h=H, **extra):
    return dict({"FR_TRACK_HISTORY": str(h)}, **extra)


def voices(g, time_slot=0):
    p = synth.voice_params(V, P, 0x5EED0002)
    leaves = synth.partial_leaves(g, p["w"], p["amp"], time_slot).reshape(V, P)
    return synth.sum_tree(g, leaves)


def env_tree():
    """Template voices x a per-voice envelope supplied as a track: a stage program reads it."""
    g = synth.GraphArrays()
    x = voices(g)
    y = g.nodes(K_MUL, V)
    g.edge(0, y, FIRST + np.arange(V, dtype=np.uint32), 0)
    g.edge(x, y, 0, 1)
    g.edge(y, 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def delay_tree(d):
    """voice + Delay(track, d) per voice."""
    g = synth.GraphArrays()
    x = voices(g)
    out = []
    for v in range(V):
        dl = g.binop(K_DELAY, IN(FIRST + v), C(np.float32(d)), 1)
        out.append(g.binop(K_SUM2, x[v:v + 1], dl, 1)[0])
    g.edge(np.array(out, dtype=np.uint32), 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def time_track_tree():
    """Template voices whose time input is a track (slot FIRST holds the ramp)."""
    g = synth.GraphArrays()
    x = voices(g, time_slot=FIRST)
    g.edge(x, 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def pull_tree():
    """Rows for the pull interpreter (mode "pull"): a track at the current frame plus a constant Delay of another."""
    g = synth.GraphArrays()
    out = []
    for v in range(V):
        dl = g.binop(K_DELAY, IN(FIRST + (v + 1) % V), C(np.float32(300.0)), 1)
        out.append(g.binop(K_SUM2, IN(FIRST + v), dl, 1)[0])
    g.edge(np.array(out, dtype=np.uint32), 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def rows(idx, T, n_tracks=V, seed=0, ramp_track=False):
    rng = np.random.default_rng(seed * 1000003 + idx)
    m = np.zeros((FIRST + n_tracks, T), np.float32)
    m[0] = synth.time_ramp(idx, idx + T)
    m[FIRST:] = rng.normal(size=(n_tracks, T)).astype(np.float32)
    if ramp_track:
        m[FIRST] = synth.time_ramp(idx, idx + T)
    return m


class Pair:
    def __init__(self, sim, oracle_lib, tree, options=None, first=FIRST, mode="auto"):
        self.hip = Renderer(sim, mode=mode, options=opts() if options is None else options)
        self.ref = Renderer(oracle_lib)
        self.hip.set_track_inputs(first)
        synth.install(self.hip, tree)
        synth.install(self.ref, tree)
        self.tree = tree

    def call(self, idx, m, n_slots=V):
        T = m.shape[1]
        got = self.hip.fill_buffer_dense(n_slots, idx, idx + T, m)
        exp = self.ref.fill_buffer_dense(n_slots, idx, idx + T, m)
        assert same_bits(got, exp), (idx, T, np.flatnonzero(got.view(np.uint32) != exp.view(np.uint32))[:8])
        return got

    def both(self, fn, *a):
        getattr(self.hip, fn)(*a)
        getattr(self.ref, fn)(*a)

    def close(self):
        self.hip.close()
        self.ref.close()


def play(pair, make_rows, calls=CALLS, seek_to=50000):
    idx = 0
    for T in calls:
        pair.call(idx, make_rows(idx, T))
        idx += T
    idx = seek_to
    for T in (64, 4800, 1):
        pair.call(idx, make_rows(idx, T))
        idx += T
    return idx


# ---- the option ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", ["0", str(1 << 24)])
def test_option_accepted(sim, clean_env, value):
    with Renderer(sim, options={"FR_TRACK_HISTORY": value}) as r:
        assert r.options()["FR_TRACK_HISTORY"] == {"value": value, "source": "option"}
    clean_env.setenv("FR_TRACK_HISTORY", value)
    with Renderer(sim) as r:
        assert r.options()["FR_TRACK_HISTORY"] == {"value": value, "source": "env"}


@pytest.mark.parametrize("value", ["-1", "x", str((1 << 24) + 1), ""])
def test_option_refused(sim, clean_env, value):
    with pytest.raises(RenderError) as ei:
        Renderer(sim, options={"FR_TRACK_HISTORY": value})
    assert ei.value.status == FR_ERR_INVALID_ARG
    clean_env.setenv("FR_TRACK_HISTORY", value)
    with pytest.raises(RenderError) as ei:
        Renderer(sim)
    assert ei.value.status == FR_ERR_INVALID_ARG


def test_option_off_keeps_todays_refusals(sim, oracle_lib, clean_env):
    for tree, mode in ((env_tree(), "auto"), (delay_tree(10), "auto"), (time_track_tree(), "auto"), (pull_tree(), "pull")):
        with Renderer(sim, mode=mode) as r:
            assert "FR_TRACK_HISTORY" not in r.options()
            r.set_track_inputs(FIRST)
            synth.install(r, tree)
            with pytest.raises(RenderError) as ei:
                r.fill_buffer_dense(V, 0, 64, rows(0, 64))
            assert ei.value.status == FR_ERR_UNSUPPORTED
    with Renderer(sim) as r:                     # a plain graph: no tail
        r.set_track_inputs(FIRST)
        synth.install(r, synth.additive_tree(V, P))
        r.fill_buffer_dense(V, 0, 64, rows(0, 64))
        p = r.plan()
        assert p["track_history"] == 0 and p["track_tail_bytes"] == 0 and p["track_tail_launches"] == 0, p


# ---- readers ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["envelope", "delay_1", "delay_H", "time_track", "pull"])
def test_readers_match_the_oracle(sim, oracle_lib, clean_env, case):
    tree = {"envelope": env_tree, "delay_1": lambda: delay_tree(1), "delay_H": lambda: delay_tree(H),
            "time_track": time_track_tree, "pull": pull_tree}[case]()
    pair = Pair(sim, oracle_lib, tree, mode="pull" if case == "pull" else "auto")
    try:
        play(pair, lambda i, T: rows(i, T, ramp_track=case == "time_track"))
        p = pair.hip.plan()
        assert p["track_history"] == H and p["track_window_slots"] >= 1, p
        assert p["track_tail_launches"] == 1 and p["track_tail_bytes"] == V * 8192 * 4, p
        if case == "delay_H":
            assert p["track_lookback"] == H, p
        if case == "pull":
            assert p["pull_rows"] == V and p["track_lookback"] == 300, p
    finally:
        pair.close()


def test_edit_adds_a_delay_into_frames_rendered_before(sim, oracle_lib, clean_env):
    """The tail is what serves this: Delay(track, H) added after several calls reads frames no call stored."""
    pair = Pair(sim, oracle_lib, env_tree())
    try:
        idx = 0
        for T in (700, 4800, 64, 4800):
            pair.call(idx, rows(idx, T))
            idx += T
        h = 100000
        pair.both("on_add_node", h, "Delay")
        pair.both("on_add_node", h + 1, "Sum2")
        pair.both("on_add_edge", 0, h, FIRST + 1, 0)
        pair.both("on_add_edge", 1, h, f32_bits(float(H)), 1)
        pair.both("on_add_edge", 0, h + 1, FIRST, 0)
        pair.both("on_add_edge", h, h + 1, 0, 1)
        pair.both("on_add_edge", h + 1, 0, 0, 0)
        for T in (1, 700, 4800):
            got = pair.call(idx, rows(idx, T))
            assert np.abs(got[0]).max() > 0
            idx += T
        assert pair.hip.plan()["track_lookback"] == H
    finally:
        pair.close()


def test_dropped_and_unsupplied_rows_read_zero(sim, oracle_lib, clean_env):
    """A first call of 1 frame: `buff.len()` = V input vectors, the last track row is dropped (the reference stores nothing
    for it).  Later a row stops being supplied.  Delays read both back through the tail."""
    pair = Pair(sim, oracle_lib, delay_tree(700))
    try:
        idx = 0
        for T in (1, 64, 700, 4800):
            pair.call(idx, rows(idx, T))
            idx += T
        for T in (64, 700, 700, 4800):            # the last track row is no longer supplied
            pair.call(idx, rows(idx, T, n_tracks=V - 1))
            idx += T
    finally:
        pair.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------

def refused_then_exact(pair, idx, add, remove, T=64, match="", make=rows):
    """`add` (on both renderers) makes the plan unservable: the call is refused and leaves the renderer as it was; after
    `remove` (on both) the same call is exact."""
    for fn, *a in add:
        pair.both(fn, *a)
    with pytest.raises(RenderError) as ei:
        pair.hip.fill_buffer_dense(V, idx, idx + T, make(idx, T))
    assert ei.value.status == FR_ERR_UNSUPPORTED, ei.value
    assert match in str(ei.value), str(ei.value)
    for fn, *a in remove:
        pair.both(fn, *a)
    pair.call(idx, make(idx, T))
    return idx + T


def warm(pair, make=rows):
    idx = 0
    for T in (700, 4800):
        pair.call(idx, make(idx, T))
        idx += T
    return idx


def delay_edits(pair, h, src, amount):
    """A Delay(src, amount) node that replaces output row 0's source; `remove` puts the old source back."""
    e = pair.tree["edges"]
    old = e[(e[:, 1] == 0) & (e[:, 3] == 0)][0]
    add = [("on_add_node", h, "Delay"), ("on_add_edge", src[0], h, src[1], 0), ("on_add_edge", amount[0], h, amount[1], 1),
           ("on_add_edge", h, 0, 0, 0)]
    remove = [("on_add_edge", int(old[0]), 0, int(old[2]), 0), ("on_del_node", h)]
    return add, remove


def test_refused_beyond_the_history(sim, oracle_lib, clean_env):
    pair = Pair(sim, oracle_lib, env_tree(), options=opts(1024))
    try:
        idx = warm(pair)
        add, remove = delay_edits(pair, 100000, (0, FIRST), (1, f32_bits(1025.0)))
        refused_then_exact(pair, idx, add, remove, match="1025 frames")
    finally:
        pair.close()


def test_refused_unbounded_delay_of_a_track(sim, oracle_lib, clean_env):
    pair = Pair(sim, oracle_lib, env_tree())
    try:
        idx = warm(pair)
        add, remove = delay_edits(pair, 100000, (0, FIRST), (0, 0))            # amount: the time ramp, no bound
        refused_then_exact(pair, idx, add, remove, match="no bound")
    finally:
        pair.close()


def test_observed_amount_reading_a_track_is_not_bounded(sim, oracle_lib, clean_env):
    """FR_DELAY_OBSERVED bounds amounts by stored values; tracks are not stored, so an amount that reads one keeps no bound:
    the Delay stays with the pull interpreter, exact."""
    pair = Pair(sim, oracle_lib, env_tree(), options=opts(H, FR_DELAY_OBSERVED="1"))
    try:
        idx = warm(pair)
        for fn, *a in [("on_add_node", 100001, "Sum2"), ("on_add_edge", 0, 100001, FIRST + 2, 0), ("on_add_edge", 1, 100001, f32_bits(5.0), 1),
                       ("on_add_node", 100000, "Delay"), ("on_add_edge", 0, 100000, 0, 0), ("on_add_edge", 100001, 100000, 0, 1),
                       ("on_add_edge", 100000, 0, 0, 0)]:
            pair.both(fn, *a)
        for T in (64, 700):
            pair.call(idx, rows(idx, T))
            idx += T
        assert pair.hip.plan()["observed_delays"] == 0
    finally:
        pair.close()


def test_readd_after_refusal_keeps_the_tail(sim, oracle_lib, clean_env):
    """A refused call did not advance the tail: the same Delay within the history renders exactly afterwards."""
    pair = Pair(sim, oracle_lib, env_tree(), options=opts(1024))
    try:
        idx = warm(pair)
        add, remove = delay_edits(pair, 100000, (0, FIRST), (1, f32_bits(2000.0)))
        idx = refused_then_exact(pair, idx, add, remove, match="2000 frames")
        h = 100001
        pair.both("on_add_node", h, "Delay")
        pair.both("on_add_edge", 0, h, FIRST, 0)
        pair.both("on_add_edge", 1, h, f32_bits(1024.0), 1)
        pair.both("on_add_edge", h, 0, 0, 1)
        for T in (1, 64, 4800):
            pair.call(idx, rows(idx, T))
            idx += T
    finally:
        pair.close()


# ---- random graphs ---------------------------------------------------------------------------------------------------------

def test_random_graphs_exact_or_refused(sim, oracle_lib, clean_env):
    """The upper half of the input slots declared tracks (full-length rows): every call either matches the oracle bit for bit
    or is refused with FR_ERR_UNSUPPORTED (then neither renderer takes the call: both see the next one as a seek)."""
    n_in, n_out, first = 4, 3, 2
    rendered = refused = 0
    for seed in range(40):
        steps, _ = randgraph.random_graph(seed, n_inputs=n_in, n_outputs=n_out)
        rng = np.random.default_rng(seed)
        hip = Renderer(sim, options=opts(64))
        ref = Renderer(oracle_lib)
        try:
            hip.set_track_inputs(first)
            randgraph.install_steps(hip, steps)
            randgraph.install_steps(ref, steps)
            idx = 0
            for k in range(8):
                if k == 4:
                    idx += 1000                                           # a seek
                if k in (3, 6):
                    edits = randgraph.random_edits(rng, steps, 3, n_inputs=n_in, n_outputs=n_out)
                    randgraph.install_steps(hip, edits)
                    randgraph.install_steps(ref, edits)
                T = int(rng.choice([1, 7, 64, 130]))
                m = rng.normal(size=(n_in, T)).astype(np.float32) * 4
                m[0] = synth.time_ramp(idx, idx + T)
                try:
                    got = hip.fill_buffer_dense(n_out, idx, idx + T, m)
                except RenderError as e:
                    assert e.status == FR_ERR_UNSUPPORTED, (seed, k, e)
                    refused += 1
                    idx += T
                    continue
                exp = ref.fill_buffer_dense(n_out, idx, idx + T, m)
                assert same_bits(got, exp), (seed, k, T)
                rendered += 1
                idx += T
        finally:
            hip.close()
            ref.close()
    assert rendered >= 200, (rendered, refused)


def test_refused_feedback_loop_reading_a_track(sim, clean_env):
    """y = track + 0.5 * Delay(y, 3): a feedback plan replays its rings from frame 0, which no bounded history can serve."""
    with Renderer(sim, options=opts()) as r:
        r.set_track_inputs(FIRST)
        for h, kind in ((1, "F32Constant"), (2, "Delay"), (3, "Multiply"), (4, "Sum2")):
            r.on_add_node(h, kind)
        for e in ((0, 4, FIRST, 0), (3, 4, 0, 1), (1, 3, f32_bits(0.5), 0), (2, 3, 0, 1), (4, 2, 0, 0), (1, 2, f32_bits(3.0), 1),
                  (4, 0, 0, 0)):
            r.on_add_edge(*e)
        with pytest.raises(RenderError) as ei:
            r.fill_buffer_dense(1, 0, 64, rows(0, 64, n_tracks=1))
        assert ei.value.status == FR_ERR_UNSUPPORTED and "feedback" in str(ei.value), ei.value
