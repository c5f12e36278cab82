"""FR_DELAY_OBSERVED on the CPU: the engine's own host code in the host-logic simulator (tests/sim_tools.py) against the
oracle, bit for bit.  A Delay whose amount comes from an input is staged (bank -> ring -> S_READ_DYN) with a look-back
bounded by the values the input has actually held since the last seek; rows that widen the bound re-plan with a larger
look-back; seeks, edits, special amounts, a capped history, Sparkle semantics and sharding keep the oracle's bits.  With the
option off the same graphs stay with the pull interpreter.  The device side is tests/test_hip_observed_delay.py."""
import numpy as np
import pytest

import sim_tools
from kat_replay import same_bits
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, RenderError, Renderer
from observed_delay_cases import (AMOUNTS, BASE, SPECIALS, DeviceRows, Pair, delayed_voices, edit_base, render, rows_for, run_growth,
                                  special_row)
from shard_harness import Mailboxes

ON = {"FR_DELAY_OBSERVED": "1"}
V, P = 3, 16


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture
def clean_env(monkeypatch):
    monkeypatch.delenv("FR_DELAY_OBSERVED", raising=False)
    monkeypatch.delenv("FR_DELAY_OBSERVED_MAX", raising=False)
    return monkeypatch


@pytest.mark.parametrize("amount", AMOUNTS)
def test_option_off_stays_with_the_pull_interpreter(sim, oracle_lib, clean_env, amount):
    pair = Pair(sim, oracle_lib, delayed_voices(V, P, amount))
    try:
        plans, _ = run_growth(pair, amount)
    finally:
        pair.close()
    for p in plans:
        assert p["pull_rows"] == V and p["observed_delays"] == 0 and not p["delay_observed"], p
        assert p["lookback_growths"] == 0 and p["range_launches"] == 0, p


@pytest.mark.parametrize("entry", ["host", "dense", "device", "device_dense"])
@pytest.mark.parametrize("amount", AMOUNTS)
def test_growing_amounts_are_staged_and_exact(sim, oracle_lib, clean_env, amount, entry):
    pair = Pair(sim, oracle_lib, delayed_voices(V, P, amount), options=ON, entry=entry)
    try:
        plans, _ = run_growth(pair, amount)
    finally:
        pair.close()
    for p in plans:
        assert p["pull_rows"] == 0 and p["observed_delays"] == V and p["delay_observed"], p
        assert p["rings"] >= 1 and p["observed_lookback"] >= 1, p
    looks = [p["observed_lookback"] for p in plans]
    assert looks == sorted(looks) and looks[-1] > looks[0], looks
    assert all(lb & (lb - 1) == 0 for lb in looks), looks               # powers of two
    growths = [p["lookback_growths"] for p in plans]
    assert growths[-1] >= 2 and growths == sorted(growths), growths
    # a growth happens exactly when the planned look-back moves
    assert growths[-1] - growths[0] == sum(1 for a, b in zip(looks, looks[1:]) if b > a), (growths, looks)
    if entry.startswith("device"):
        assert plans[-1]["range_launches"] > 0, plans[-1]
    else:
        assert plans[-1]["range_launches"] == 0, plans[-1]


def test_seek_rebuilds_and_may_shrink(sim, oracle_lib, clean_env):
    pair = Pair(sim, oracle_lib, delayed_voices(V, P, "in"), options=ON)
    try:
        plans, t = run_growth(pair, "in")
        big = plans[-1]["observed_lookback"]
        assert big >= 2048
        p = pair.call(700, 956, rows_for(700, 956, 1.0, 20.0), "backward seek")
        assert p["observed_lookback"] == 32 and p["pull_rows"] == 0, p
        p = pair.call(956, 1212, rows_for(956, 1212, 0.0, 300.0), "growth after the seek")
        assert p["observed_lookback"] == 512, p
        p = pair.call(50000, 50256, rows_for(50000, 50256, 0.0, 2.0), "forward seek")
        assert p["observed_lookback"] == 2, p
        p = pair.call(50256, 50512, rows_for(50256, 50512, 3.0, 4.0), "contiguous")
        assert p["observed_lookback"] == 4, p
    finally:
        pair.close()


def test_edit_replans_with_the_hull_kept(sim, oracle_lib, clean_env):
    tree = delayed_voices(V, P, "affine")
    pair = Pair(sim, oracle_lib, tree, options=ON)
    try:
        plans, t = run_growth(pair, "affine")
        before = plans[-1]["plans_built"]
        edit_base([pair.r, pair.ref], tree, np.float32(BASE), np.float32(5000.0))
        p = pair.call(t, t + 256, rows_for(t, t + 256, 0.0, 1.0), "after the edit")
        assert p["plans_built"] > before and p["pull_rows"] == 0 and p["observed_delays"] == V, p
        assert p["observed_lookback"] == 8192, p     # base 5000 + 300 * (the 9.x the slot held before the edit)
        p = pair.call(t + 256, t + 512, rows_for(t + 256, t + 512, 0.0, 1.0), "steady after the edit")
        assert p["plans_built"] == pair.r.plan()["plans_built"]
    finally:
        pair.close()


def test_edit_adding_an_observed_delay_reads_the_stored_history(sim, oracle_lib, clean_env):
    """A slot that no observed amount read is not scanned as rows arrive; the plan that first reads it reduces its stored history."""
    g = synth.GraphArrays()
    p = synth.voice_params(1, 8, 77, False)
    x = synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"], 0).reshape(1, 8))
    g.edge(x, 0, 0, 0)
    tree = g.finish(1)
    pair = Pair(sim, oracle_lib, tree, options=ON, entry="device")
    try:
        t = 0
        for k, hi in enumerate([10.0, 900.0, 40.0]):
            pl = pair.call(t, t + 256, rows_for(t, t + 256, 0.0, hi, k), "no observed amount yet")
            t += 256
        assert pl["range_launches"] == 0 and pl["observed_delays"] == 0, pl
        dl = int(x[0]) + 1000
        for r in (pair.r, pair.ref):
            r.on_add_node(dl, synth.Effect.primitive("Delay"))
            r.on_add_edge(int(x[0]), dl, 0, 0)
            r.on_add_edge(0, dl, 1, 1)          # amount = input slot 1
            r.on_del_edge(int(x[0]), 0, 0, 0)
            r.on_add_edge(dl, 0, 0, 0)
        pl = pair.call(t, t + 256, rows_for(t, t + 256, 0.0, 5.0), "after adding the Delay")
        assert pl["observed_delays"] == 1 and pl["pull_rows"] == 0 and pl["range_launches"] >= 1, pl
        assert pl["observed_lookback"] == 1024, pl    # the 900.x stored two calls earlier
    finally:
        pair.close()


@pytest.mark.parametrize("label,values", SPECIALS, ids=[s[0] for s in SPECIALS])
@pytest.mark.parametrize("amount", ["in", "affine"])
def test_special_amounts(sim, oracle_lib, clean_env, amount, label, values):
    pair = Pair(sim, oracle_lib, delayed_voices(V, P, amount), options=ON)
    try:
        t = 0
        for n in (256, 300, 256):
            pl = pair.call(t, t + n, [synth.time_ramp(t, t + n), special_row(t, t + n, values)], f"{label} at {t}")
            t += n
        # ("beyond_t" under "affine": 100 + 300 * 1e6 frames is more than FR_DELAY_OBSERVED_MAX; -inf times 300 has no bound)
        bounded = label in ("nan", "neg") or (label in ("neg_inf", "beyond_t") and amount == "in")
        if bounded:
            assert pl["pull_rows"] == 0 and pl["observed_delays"] == V, pl
        else:
            assert pl["pull_rows"] == V and pl["observed_refused"] == V, pl
        # a seek forgets the special values: the amounts are staged again
        pl = pair.call(100, 356, rows_for(100, 356, 0.0, 50.0), "seek")
        assert pl["pull_rows"] == 0 and pl["observed_delays"] == V, pl
        assert pl["observed_lookback"] == (64 if amount == "in" else 16384), pl     # 50.x, or 100 + 300 * 50.x
    finally:
        pair.close()


def test_history_frames(sim, oracle_lib, clean_env):
    pair = Pair(sim, oracle_lib, delayed_voices(V, P, "in"), options=ON, history_frames=8192)
    try:
        plans, t = run_growth(pair, "in")
        for k in range(30):   # the buffer slides
            pl = pair.call(t, t + 512, rows_for(t, t + 512, 0.0, 3000.0, k), f"slide {k}")
            t += 512
        assert pl["history_frames"] == 8192 and pl["pull_rows"] == 0 and pl["observed_lookback"] == 4096, pl
        assert pl["input_lookback"] >= 4096, pl
    finally:
        pair.close()


def test_sparkle_semantics(sim, oracle_lib, clean_env):
    pair = Pair(sim, oracle_lib, delayed_voices(V, P, "in"), options=ON, semantics="sparkle")
    try:
        plans, t = run_growth(pair, "in")
        pl = pair.call(t, t + 256, [synth.time_ramp(t, t + 256), special_row(t, t + 256, [np.nan, -3.0, 5.0, 100.5])], "sparkle specials")
        assert pl["pull_rows"] == 0 and pl["observed_delays"] == V, pl
    finally:
        pair.close()


def test_observed_max_falls_back_to_pull(sim, oracle_lib, clean_env):
    pair = Pair(sim, oracle_lib, delayed_voices(V, P, "in"), options={"FR_DELAY_OBSERVED": "1", "FR_DELAY_OBSERVED_MAX": "1024"})
    try:
        pl = pair.call(0, 256, rows_for(0, 256, 0.0, 1000.0), "within the maximum")
        assert pl["pull_rows"] == 0 and pl["observed_lookback"] == 1024 and pl["delay_observed_max"] == 1024, pl
        pl = pair.call(256, 512, rows_for(256, 512, 0.0, 1500.0), "beyond the maximum")
        assert pl["pull_rows"] == V and pl["observed_refused"] == V and pl["observed_delays"] == 0, pl
        pl = pair.call(512, 768, rows_for(512, 768, 0.0, 10.0), "still beyond (the hull keeps 1500)")
        assert pl["pull_rows"] == V, pl
        pl = pair.call(0, 256, rows_for(0, 256, 0.0, 10.0), "seek")
        assert pl["pull_rows"] == 0 and pl["observed_lookback"] == 16, pl
    finally:
        pair.close()


@pytest.mark.parametrize("name,value", [("FR_DELAY_OBSERVED", "2"), ("FR_DELAY_OBSERVED", "-1"), ("FR_DELAY_OBSERVED", ""),
                                        ("FR_DELAY_OBSERVED", "on"), ("FR_DELAY_OBSERVED_MAX", "1023"),
                                        ("FR_DELAY_OBSERVED_MAX", "268435457"), ("FR_DELAY_OBSERVED_MAX", "1e6"),
                                        ("FR_DELAY_OBSERVED_MAX", "0")])
def test_invalid_options_are_refused(sim, clean_env, name, value):
    with pytest.raises(RenderError) as e:
        Renderer(sim, options={name: value})
    assert e.value.status == FR_ERR_INVALID_ARG


def test_options_and_environment(sim, clean_env):
    with Renderer(sim) as r:
        synth.install(r, delayed_voices(1, 8, "in"))
        r.fill_buffer(1, 0, 64, rows_for(0, 64, 0.0, 1.0))
        p = r.plan()
        assert not p["delay_observed"] and p["delay_observed_max"] == 1 << 20, p
        assert "FR_DELAY_OBSERVED" not in r.options()     # (a rendering mode: fr_plan_json reports it, not the tuning switches)
    clean_env.setenv("FR_DELAY_OBSERVED", "1")
    clean_env.setenv("FR_DELAY_OBSERVED_MAX", "5")        # the environment's lenient reading: clamped to 1024
    with Renderer(sim) as r, Renderer(sim, options={"FR_DELAY_OBSERVED": "0"}) as off:
        for x in (r, off):
            synth.install(x, delayed_voices(1, 8, "in"))
            x.fill_buffer(1, 0, 64, rows_for(0, 64, 0.0, 1.0))
        assert r.plan()["delay_observed"] and r.plan()["delay_observed_max"] == 1024 and r.plan()["pull_rows"] == 0
        assert not off.plan()["delay_observed"] and off.plan()["pull_rows"] == 1


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("mode", ["voices", "partials"])
def test_sharded_ranks_plan_alike(sim, oracle_lib, clean_env, mode, world):
    import threading
    Vs = 5
    tree = delayed_voices(Vs, 32, "affine")
    boxes = Mailboxes(world)
    ranks = [Renderer(sim, options=ON) for _ in range(world)]
    ref = Renderer(oracle_lib)
    try:
        for k, r in enumerate(ranks):
            r.set_shard(k, world, mode, sendrecv=boxes.transport(k))
            synth.install(r, tree)
        synth.install(ref, tree)
        t = 0
        for c, (n, lo, hi) in enumerate([(256, 0.0, 0.5), (256, 0.0, 3.0), (300, 1.0, 9.0), (256, 0.0, 2.0)]):
            rows = rows_for(t, t + n, lo, hi, c)
            outs, plans, errs = [None] * world, [None] * world, []

            def run(k):
                try:
                    outs[k] = ranks[k].fill_buffer(Vs, t, t + n, rows, out=np.full((Vs, n), -7.0, np.float32))
                    plans[k] = ranks[k].plan()
                except BaseException as e:  # noqa: BLE001
                    errs.append(e)
            th = [threading.Thread(target=run, args=(k,)) for k in range(world)]
            for x in th:
                x.start()
            for x in th:
                x.join(300)
            assert not errs, errs
            exp = ref.fill_buffer(Vs, t, t + n, rows)
            got = np.empty_like(exp)
            for k, r in enumerate(ranks):
                lo_, hi_ = r.shard_rows(Vs)
                got[lo_:hi_] = outs[k][lo_:hi_]
            assert same_bits(got, exp), f"call {c}"
            for pl in plans:
                assert pl["pull_rows"] == 0, pl
            looks = {(pl["observed_lookback"], pl["lookback_growths"], pl["max_lookback"]) for pl in plans}
            assert len(looks) == 1, looks     # every rank saw the same rows: same bounds, same plan
            if mode == "partials":
                assert len({(pl["observed_delays"], pl["shard"]["split_voices"], pl["rings"]) for pl in plans}) == 1, plans
            t += n
        assert plans[0]["lookback_growths"] >= 2
    finally:
        for r in ranks:
            r.close()
        ref.close()
