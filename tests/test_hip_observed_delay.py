"""FR_DELAY_OBSERVED on an MI355X: the cases of tests/test_observed_delay_sim.py on libfriendship_hip.so through host rows,
device rows (input_range_kernel reduces them: range_launches > 0) and dense calls, with the compiled stage programs on and
off, and one full-size case -- 128 voices x 1024 partials, 4800-frame calls, Delay(voice, base + depth * In(1)) -- sampled
against the oracle across a growth of the look-back."""
import numpy as np
import pytest

import oracle_tools
from kat_replay import same_bits
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer
from observed_delay_cases import AMOUNTS, SPECIALS, Pair, delayed_voices, rows_for, run_growth, special_row

pytestmark = pytest.mark.gpu

ON = {"FR_DELAY_OBSERVED": "1"}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("stage_jit", ["0", "1"])
@pytest.mark.parametrize("entry", ["host", "dense", "device", "device_dense"])
@pytest.mark.parametrize("amount", AMOUNTS)
def test_growing_amounts(hip_lib, oracle_lib, amount, entry, stage_jit):
    V, P = 4, 64
    pair = Pair(hip_lib, oracle_lib, delayed_voices(V, P, amount), options=dict(ON, FR_STAGE_JIT=stage_jit), entry=entry)
    try:
        plans, t = run_growth(pair, amount)
        pl = pair.call(300, 556, rows_for(300, 556, 0.0, 3.0), "seek")
        assert pl["pull_rows"] == 0 and pl["observed_delays"] == V, pl
    finally:
        pair.close()
    for p in plans:
        assert p["pull_rows"] == 0 and p["observed_delays"] == V, p
    assert plans[-1]["lookback_growths"] >= 2, plans[-1]
    assert (plans[-1]["range_launches"] > 0) == entry.startswith("device"), plans[-1]


def test_option_off_pulls(hip_lib, oracle_lib):
    pair = Pair(hip_lib, oracle_lib, delayed_voices(2, 32, "affine"))
    try:
        plans, _ = run_growth(pair, "affine")
    finally:
        pair.close()
    assert all(p["pull_rows"] == 2 and p["observed_delays"] == 0 for p in plans)


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("label,values", SPECIALS, ids=[s[0] for s in SPECIALS])
def test_special_amounts(hip_lib, oracle_lib, label, values, entry):
    V = 3
    pair = Pair(hip_lib, oracle_lib, delayed_voices(V, 32, "in"), options=ON, entry=entry)
    try:
        t = 0
        for n in (256, 300):
            pl = pair.call(t, t + n, [synth.time_ramp(t, t + n), special_row(t, t + n, values)], label)
            t += n
        assert pl["pull_rows"] == (V if label in ("pos_inf", "2^64") else 0), pl
        pl = pair.call(64, 320, rows_for(64, 320, 0.0, 50.0), "seek")
        assert pl["pull_rows"] == 0 and pl["observed_lookback"] == 64, pl
    finally:
        pair.close()


def test_history_frames_and_sparkle(hip_lib, oracle_lib):
    for kw in ({"history_frames": 8192}, {"semantics": "sparkle"}):
        pair = Pair(hip_lib, oracle_lib, delayed_voices(3, 64, "in"), options=ON, entry="device", **kw)
        try:
            plans, t = run_growth(pair, "in")
            for k in range(12):
                pl = pair.call(t, t + 1024, rows_for(t, t + 1024, 0.0, 3000.0, k), f"{kw} {k}")
                t += 1024
            assert pl["pull_rows"] == 0 and pl["observed_lookback"] == 4096, pl
        finally:
            pair.close()


@pytest.mark.timeout(900)
def test_full_size_sampled_against_oracle_across_a_growth(hip_lib, oracle_lib):
    """128 voices x 1024 partials, Delay(voice, 100 + 300 * In(1)), five contiguous 4800-frame calls whose control rows widen
    (look-back 1024 -> 4096 -> 32768 at the third call), then a backward seek; 32 voices x ~40 frames against the oracle,
    which answers single samples from the stored input history."""
    V, P, T = 128, 1024, 4800
    tree = delayed_voices(V, P, "affine", seed=11)
    spans = [(0.0, 2.0), (0.0, 9.0), (5.0, 90.0), (0.0, 90.0), (20.0, 30.0)]
    calls = [(k * T, rows_for(k * T, (k + 1) * T, lo, hi, k)) for k, (lo, hi) in enumerate(spans)]
    with Renderer(hip_lib, options=ON) as hip, Renderer(oracle_lib) as ref:
        synth.install(hip, tree)
        got, plans = [], []
        for st, rows in calls:
            got.append((st, hip.fill_buffer(V, st, st + T, rows)))
            plans.append(hip.plan())
        assert all(p["pull_rows"] == 0 and p["observed_delays"] == V for p in plans), plans[-1]
        looks = [p["observed_lookback"] for p in plans]
        assert looks == [1024, 4096, 32768, 32768, 32768], looks
        # (the first call's plan is made before its rows are stored, from an empty history: its rows are a growth too)
        assert plans[-1]["lookback_growths"] == 3, plans[-1]
        # the oracle: graph without its output edges, the calls' rows stored, then the outputs connected
        e = tree["edges"]
        synth.install(ref, dict(tree, edges=e[e[:, 1] != 0]))
        for st, rows in calls:
            assert not ref.fill_buffer(1, st, st + T, rows).any()
        ref.on_add_edges(e[e[:, 1] == 0])
        rng = np.random.default_rng(5)
        voices = np.unique(np.concatenate([[0, 1, 63, 127], rng.integers(0, V, 40)]))[:32]
        frames = np.unique(np.concatenate([[0, 1, 1023, 1024, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 2 * T + 1000, 3 * T - 1, 3 * T, 4 * T,
                                            5 * T - 1], rng.integers(0, 5 * T, 25)]))
        slots, times = np.repeat(voices, len(frames)).astype(np.uint32), np.tile(frames, len(voices)).astype(np.uint64)
        exp = oracle_tools.eval_samples(ref, slots, times).reshape(len(voices), len(frames))
        g = np.empty_like(exp)
        for j, f in enumerate(frames):
            st, arr = next((s, a) for s, a in got if s <= f < s + a.shape[1])
            g[:, j] = arr[voices, int(f) - st]
        assert same_bits(g, exp), np.argwhere(g.view(np.uint32) != exp.view(np.uint32))[:8].tolist()
        assert np.abs(g).max() > 0.01
