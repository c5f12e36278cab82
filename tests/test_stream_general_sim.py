"""FR_STREAM_GENERAL on the CPU: the serving rule of block streaming for voices of any partial count (csrc/streamplan.hpp)
through the engine's own host code in the host-logic simulator.  With FR_STREAM_PROGRAMS and FR_STREAM_GENERAL on,
fr_plan_json's "stream" lists the leaf count of every voice served by schedule ("general_voices") and the limit, and names the
kernel.  The simulator has no resident launches: the kernel itself is tests/test_hip_stream_general.py; the schedule validation,
the chunk dealing and a host model of the kernel's schedule renderer are tests/test_stream_general_host.py."""
import numpy as np
import pytest

import sim_tools
import stream_banks_cases as M
import stream_cases as K
import stream_general_cases as G
import stream_loop_cases as L
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, FR_ERR_UNSUPPORTED, RenderError, Renderer


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture(scope="module")
def trees():
    """Every case's graph, built once."""
    t = {c["name"]: c["build"]() for c in G.SERVABLE}
    t.update({c[0]: c[1]() for c in G.REFUSED})
    return t


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_LOOP_TILES", "FR_RING_KEEP",
              "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def plan_of(sim, tree, n_rows, options, n_in=1):
    with Renderer(sim, options=options) as r:
        synth.install(r, tree)
        r.fill_buffer(n_rows, 0, 64, [synth.time_ramp(0, 64)] + [np.ones(64, np.float32)] * (n_in - 1))
        assert ("FR_STREAM_GENERAL" in r.options()) == ("FR_STREAM_GENERAL" in options)
        return r.plan()


def without(options):
    return {k: v for k, v in options.items() if k != "FR_STREAM_GENERAL"}


def strip(s):
    """The stream object without what the option adds."""
    s = {k: v for k, v in s.items() if k not in G.NEW_KEYS}
    if "banks" in s:
        s["banks"] = [{k: v for k, v in b.items() if k != "general"} for b in s["banks"]]
    return s


@pytest.mark.parametrize("name", [c["name"] for c in G.SERVABLE])
def test_servable_with_the_option(sim, clean_env, trees, name):
    c = G.case(name)
    plan = plan_of(sim, trees[name], c["n_rows"], c["options"], c["n_in"])
    s = plan["stream"]
    G.check_stream_object(s, c)
    with Renderer(sim, options=c["options"]) as r:                   # fr_stream_begin builds the tables (the simulator launches nothing)
        synth.install(r, trees[name])
        r.stream_begin(c["n_rows"])
        with pytest.raises(RenderError):
            r.stream_block_rows(0, [synth.time_ramp(0, 8)] * len(s["input_slots"]))
        r.fill_buffer(c["n_rows"], 0, 16, [synth.time_ramp(0, 16)] * c["n_in"])


def test_the_leaf_counts_in_voice_order(sim, clean_env, trees):
    for name, leaves in (("additive_2x100", [100, 100]), ("additive_1x3000", [3000]), ("additive_2x32", [32, 32]), ("left_chain_20", [20, 20]),
                         ("3_plus_128", [131, 131])):
        c = G.case(name)
        s = plan_of(sim, trees[name], c["n_rows"], c["options"])["stream"]
        assert s["general_voices"] == leaves and s["programs_per_voice"] == [0] * len(leaves) and s["rings"] == 0, (name, s)


def test_a_schedule_bank_next_to_other_banks_needs_stream_banks(sim, clean_env, trees):
    c = G.case("mixed_banks")
    s = plan_of(sim, trees[c["name"]], c["n_rows"], G.OPTION)["stream"]
    assert s["servable"] is False and s["reason"] == M.old_reason(3), s
    assert s["general_voices"] == [] and s["kernel"] != G.NEW_KERNEL


@pytest.mark.parametrize("name", [c[0] for c in G.REFUSED])
def test_refused_with_the_option(sim, clean_env, trees, name):
    _, _, n_rows, options, why = K.case(G.REFUSED, name)
    s = plan_of(sim, trees[name], n_rows, options)["stream"]
    assert s["servable"] is False and all(w in s["reason"] for w in why), s
    assert s["kernel"] != G.NEW_KERNEL and s["general_voices"] == [] and s["general_max_leaves"] == G.MAX_LEAVES
    assert "general" not in s["reason"]                              # the text names only what is still refused
    with Renderer(sim, options=options) as r:
        synth.install(r, trees[name])
        with pytest.raises(RenderError) as ei:
            r.stream_begin(n_rows)
        assert ei.value.status == FR_ERR_UNSUPPORTED and all(w in str(ei.value) for w in why)
        r.fill_buffer(n_rows, 0, 16, [synth.time_ramp(0, 16)])


@pytest.mark.parametrize("name,reason", [("additive_2x100", G.OLD_GENERAL), ("additive_2x64", G.OLD_SMALL), ("comb_5_2x100", G.OLD_GENERAL)])
@pytest.mark.parametrize("off", [None, "0"])
def test_without_the_option_the_reasons_are_today_s(sim, clean_env, trees, name, reason, off):
    c = G.case(name)
    options = without(c["options"]) if off is None else dict(c["options"], FR_STREAM_GENERAL=off)
    s = plan_of(sim, trees[name], c["n_rows"], options)["stream"]
    assert s["servable"] is False and s["reason"] == reason and s["kernel"] != G.NEW_KERNEL, s
    if off is None:
        assert not any(k in s for k in G.NEW_KEYS)
        with Renderer(sim, options=options) as r:
            assert "FR_STREAM_GENERAL" not in r.options()
            synth.install(r, trees[name])
            with pytest.raises(RenderError) as ei:
                r.stream_begin(c["n_rows"])
            assert ei.value.status == FR_ERR_UNSUPPORTED
            assert reason in str(ei.value) or "block streaming needs balanced template voices, one per output row" in str(ei.value)


def _older_cases():
    for c in L.SERVABLE:
        yield "loops/" + c["name"], c["build"], c["n_rows"], c["options"], c["n_in"]
    for name, build, n_rows, options, _, _, _, slots in M.SERVABLE:
        yield "banks/" + name, build, n_rows, options, len(slots)


@pytest.mark.parametrize("case", list(_older_cases()), ids=lambda c: c[0])
def test_the_older_plans_keep_their_stream_object(sim, clean_env, case):
    """Every servable case of stream_loop_cases and stream_banks_cases: with the option on, the object it has with the option
    off plus the new keys -- kernel name included."""
    _, build, n_rows, options, n_in = case
    tree = build()
    a = plan_of(sim, tree, n_rows, options, n_in)["stream"]
    b = plan_of(sim, tree, n_rows, dict(options, FR_STREAM_GENERAL="1"), n_in)["stream"]
    assert a["servable"] is True and not any(k in a for k in G.NEW_KEYS) and not any("general" in bk for bk in a.get("banks", []))
    assert strip(b) == a and list(strip(b)) == list(a)
    assert b["general_voices"] == [] and b["general_max_leaves"] == G.MAX_LEAVES and b["kernel"] != G.NEW_KERNEL
    assert all(bk["general"] is False for bk in b.get("banks", []))


def test_the_older_refusals_keep_their_text(sim, clean_env):
    """stream_banks_cases' plan with a general voice: today's reason without the option, served with it."""
    _, build, n_rows, _, why = M.case(M.REFUSED, "with_general_voice")
    tree = build()
    a = plan_of(sim, tree, n_rows, M.OPTION)["stream"]
    assert a["servable"] is False and a["reason"] == why == G.OLD_GENERAL
    b = plan_of(sim, tree, n_rows, dict(M.OPTION, FR_STREAM_GENERAL="1"))["stream"]
    assert b["servable"] is True and b["kernel"] == G.NEW_KERNEL and b["general_voices"] == [1000], b
    for name in ("nine_sizes", "too_many_voices"):
        _, build, n_rows, _, why = M.case(M.REFUSED, name)
        tree = build()
        a = plan_of(sim, tree, n_rows, M.OPTION)["stream"]
        b = plan_of(sim, tree, n_rows, dict(M.OPTION, FR_STREAM_GENERAL="1"))["stream"]
        assert a["servable"] is False and why in a["reason"] and b["reason"] == a["reason"], (name, a, b)


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_STREAM_GENERAL" not in r.options()
    with Renderer(sim, options=G.OPTION) as r:
        assert r.options()["FR_STREAM_GENERAL"] == {"value": "1", "source": "option"}
    clean_env.setenv("FR_STREAM_GENERAL", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_STREAM_GENERAL"] == {"value": "1", "source": "env"}
        assert "FR_STREAM_PROGRAMS" not in r.options()
    with Renderer(sim, options={"FR_STREAM_GENERAL": "0"}) as r:       # the option beats the environment
        assert r.options()["FR_STREAM_GENERAL"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_STREAM_GENERAL", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_STREAM_GENERAL": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_STREAM_GENERAL", bad)                     # the environment is read as strictly
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


def test_inert_without_stream_programs(sim, clean_env, trees):
    tree = trees["additive_2x100"]
    assert "stream" not in plan_of(sim, tree, 2, {"FR_STREAM_GENERAL": "1"})
    with Renderer(sim, options={"FR_STREAM_GENERAL": "1"}) as r:
        synth.install(r, tree)
        with pytest.raises(RenderError) as ei:
            r.stream_begin(2)
        assert ei.value.status == FR_ERR_UNSUPPORTED and "block streaming needs balanced template voices, one per output row" in str(ei.value)
