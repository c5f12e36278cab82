"""FR_TRACK_HISTORY on the MI355X: track voices (per-partial w / amp as track rows, read by the generated leaves) under a
per-voice envelope track and a delay chain -- the track voices feed delay lines, so after a seek, an edit or a ring growth
their window starts before the call and is rendered from the track history -- against the CPU oracle, which gets the same
rows as ordinary inputs.  Steady state is the launch of today.  The CPU side is tests/test_track_history_sim.py."""
import numpy as np
import pytest

from kat_replay import same_bits
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer, f32_bits
from libfriendship_amd.synth import IN, K_DELAY, K_MUL, K_SUM2, C

pytestmark = pytest.mark.gpu

H = 2048
V, P = 16, 256
FIRST = 1


def first_diff(a, b):
    bad = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
    if not len(bad):
        return "equal"
    i = bad[0]
    return f"{len(bad)} differ; first at {np.unravel_index(i, a.shape)}: {a.ravel()[i]!r} vs {b.ravel()[i]!r}"


def patch():
    """track_tree(V, P) x an envelope track per voice -> delay_chain(taps=2, base_delay=300)."""
    g = synth.GraphArrays()
    n = V * P
    w_slots = FIRST + 2 * np.arange(n, dtype=np.uint32)
    leaves = synth.track_leaves(g, w_slots, w_slots + 1).reshape(V, P)
    roots = synth.sum_tree(g, leaves)
    env_first = FIRST + 2 * n
    y = g.nodes(K_MUL, V)
    g.edge(0, y, env_first + np.arange(V, dtype=np.uint32), 0)
    g.edge(roots, y, 0, 1)
    x = synth.delay_chain(g, y, taps=2, base_delay=300.0)
    g.edge(x, 0, 0, np.arange(V, dtype=np.uint32))
    t = g.finish(V)
    t["n_inputs"] = env_first + V
    t["env_first"] = env_first
    t["outs"] = x
    return t


def rows(tree, idx, T):
    m = np.zeros((tree["n_inputs"], T), np.float32)
    m[:tree["env_first"]] = synth.track_rows(V, P, idx, idx + T)
    t = np.arange(idx, idx + T, dtype=np.float64)[None, :]
    m[tree["env_first"]:] = (0.5 + 0.5 * np.cos(t / 700.0 + np.arange(V)[:, None])).astype(np.float32)
    return m


class Device:
    """fill_buffer_device_dense from host arrays (torch tensors on cuda:0)."""

    def __init__(self, r):
        import torch
        self.torch, self.r = torch, r

    def __call__(self, n_slots, start, end, m, out=None):
        torch = self.torch
        T = end - start
        d_m = torch.from_numpy(np.ascontiguousarray(m)).cuda()
        d_o = torch.empty((n_slots, T), dtype=torch.float32, device="cuda")
        s = torch.cuda.current_stream()
        self.r.fill_buffer_device_dense(d_o.data_ptr(), n_slots, T, start, d_m.data_ptr(), m.shape[0], s.cuda_stream)
        s.synchronize()
        return d_o.cpu().numpy()


def add_third_tap(r, tree):
    """Edit during playback: voice 0 gets y + 0.125 * Delay(y, 900) on top of its chain (look-back 300 + 600 + 900)."""
    h = 1 << 24
    out0 = int(tree["outs"][0])
    r.on_add_node(h, "Delay")
    r.on_add_node(h + 1, "Multiply")
    r.on_add_node(h + 2, "Sum2")
    r.on_add_edge(out0, h, 0, 0)
    r.on_add_edge(1, h, f32_bits(900.0), 1)
    r.on_add_edge(1, h + 1, f32_bits(0.125), 0)
    r.on_add_edge(h, h + 1, 0, 1)
    r.on_add_edge(out0, h + 2, 0, 0)
    r.on_add_edge(h + 1, h + 2, 0, 1)
    r.on_add_edge(h + 2, 0, 0, 0)


def play(fill_hip, hip, ref, tree):
    """Calls of 4800, 64, 1, 4800 frames, a seek, an edit mid-play, a call longer than any before (ring growth)."""
    import oracle_tools
    oracle_tools.set_threads(ref, 16)
    plans = []

    def call(idx, T):
        m = rows(tree, idx, T)
        got = fill_hip(V, idx, idx + T, m)
        exp = ref.fill_buffer_dense(V, idx, idx + T, m)
        assert same_bits(got, exp), (idx, T, first_diff(got, exp))
        assert np.abs(got).max() > 0
        plans.append(hip.plan())
        return idx + T

    idx = 0
    for T in (4800, 64, 1, 4800):
        idx = call(idx, T)
    idx = 30000
    for T in (64, 4800):
        idx = call(idx, T)
    add_third_tap(hip, tree)
    add_third_tap(ref, tree)
    for T in (700, 9600, 64):
        idx = call(idx, T)
    return plans


@pytest.mark.parametrize("stage_jit", ["0", "1"])
@pytest.mark.parametrize("entry", ["dense", "device_dense"])
def test_track_voices_feeding_delays(hip_lib, oracle_lib, entry, stage_jit):
    tree = patch()
    with Renderer(hip_lib, options={"FR_TRACK_HISTORY": str(H), "FR_STAGE_JIT": stage_jit}) as hip, Renderer(oracle_lib) as ref:
        hip.set_track_inputs(FIRST)
        synth.install(hip, tree)
        synth.install(ref, tree)
        fill = hip.fill_buffer_dense if entry == "dense" else Device(hip)
        plans = play(fill, hip, ref, tree)
    last = plans[-1]
    assert any(b["tracks"] and b["to_ring"] for b in last["banks"]), last["banks"]
    assert last["track_history"] == H and last["track_lookback"] <= H and last["track_tail_launches"] == 1, last
    assert last["track_tail_bytes"] == (tree["n_inputs"] - FIRST) * H * 4, last


def test_steady_state_launch_is_todays(hip_lib):
    """A plain track tree at T = 4800: the same bank launches and the same bits with the option off and on, one tail append
    per call."""
    import torch
    Vs, Ps, T = 64, 1024, 4800
    tree = synth.track_tree(Vs, Ps)
    R = tree["n_inputs"]
    results = {}
    for opt in ("0", "1024"):
        with Renderer(hip_lib, options={"FR_TRACK_HISTORY": opt}) as r:
            r.set_track_inputs(tree["first_track"])
            synth.install(r, tree)
            s = torch.cuda.current_stream()
            outs, launches = [], []
            idx = 0
            for k in range(3):
                m = torch.from_numpy(synth.track_rows(Vs, Ps, idx, idx + T)).cuda()
                d_o = torch.empty((Vs, T), dtype=torch.float32, device="cuda")
                r.fill_buffer_device_dense(d_o.data_ptr(), Vs, T, idx, m.data_ptr(), R, s.cuda_stream)
                s.synchronize()
                outs.append(d_o.cpu().numpy())
                p = r.plan()
                launches.append(p["bank_launches"])
                assert p["track_tail_launches"] == (1 if opt != "0" else 0), p
                idx += T
            results[opt] = (outs, launches)
    for a, b in zip(results["0"][0], results["1024"][0]):
        assert same_bits(a, b)
    assert results["0"][1] == results["1024"][1]


def test_track_voices_feeding_delays_under_voice_sharding(hip_lib, oracle_lib, monkeypatch):
    """The first case on two ranks sharing the test GPU, each rendering its block of voices (no exchange)."""
    import shard_harness
    monkeypatch.setenv("FR_TRACK_HISTORY", str(H))
    tree = patch()
    job = shard_harness.Job(hip_lib, 2, "voices")
    try:
        with Renderer(oracle_lib) as ref:
            synth.install(ref, tree)
            for ren in job.ranks:
                ren.set_track_inputs(FIRST)
                synth.install(ren, tree)

            def fill(n_slots, start, end, m):
                def one(_r, ren):
                    out = np.full((n_slots, end - start), np.float32(-12345.0), dtype=np.float32)
                    return ren.fill_buffer_dense(n_slots, start, end, m, out=out)
                return job.assemble(job.each(one), n_slots)

            class Both:   # the edit goes to every rank
                def on_add_node(self, *a):
                    for ren in job.ranks:
                        ren.on_add_node(*a)

                def on_add_edge(self, *a):
                    for ren in job.ranks:
                        ren.on_add_edge(*a)

                def plan(self):
                    return job.ranks[0].plan()
            play(fill, Both(), ref, tree)
        assert sum(job.boxes.messages) == 0
    finally:
        job.close()
