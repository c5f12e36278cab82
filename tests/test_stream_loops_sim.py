"""FR_STREAM_LOOPS on the CPU: the serving rule of block streaming for feedback loops shorter than a block
(csrc/streamplan.hpp) through the engine's own host code in the host-logic simulator.  With FR_STREAM_PROGRAMS and
FR_STREAM_LOOPS on, fr_plan_json's "stream" lists the stride of every streamed program ("loop_programs", 0 for a program that
is no loop) and the two limits, and names the kernel.  The simulator has no resident launches: the kernel itself is
tests/test_hip_stream_loops.py; the helper, a host model of the kernel's three phases and the one refusal no graph reaches (a
short read of a ring that a LATER program stores: the planner orders producers first) are tests/test_stream_loops_host.py."""
import numpy as np
import pytest

import sim_tools
import stream_bus_cases as B
import stream_cases as K
import stream_loop_cases as L
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, FR_ERR_UNSUPPORTED, RenderError, Renderer

NEW_KEYS = ("loop_programs", "loop_loads", "loop_stores")


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture(scope="module")
def trees():
    """Every case's graph, built once."""
    t = {c["name"]: c["build"]() for c in L.SERVABLE}
    t.update({c[0]: c[1]() for c in L.REFUSED})
    return t


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_LOOP_TILES", "FR_RING_KEEP", "FR_TRACK_HISTORY",
              "FR_DELAY_OBSERVED"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def plan_of(sim, tree, n_rows, options, n_in=1):
    with Renderer(sim, options=options) as r:
        synth.install(r, tree)
        r.fill_buffer(n_rows, 0, 64, [synth.time_ramp(0, 64)] + [np.ones(64, np.float32)] * (n_in - 1))
        assert ("FR_STREAM_LOOPS" in r.options()) == ("FR_STREAM_LOOPS" in options)
        return r.plan()


def without(options):
    return {k: v for k, v in options.items() if k != "FR_STREAM_LOOPS"}


@pytest.mark.parametrize("tiles", [None, "1"])
@pytest.mark.parametrize("name", [c["name"] for c in L.SERVABLE])
def test_servable_with_the_option(sim, clean_env, trees, name, tiles):
    """... whatever FR_LOOP_TILES says: the rule computes the stride itself, and the carry annotations the plan carries are not
    what the stream runs."""
    c = L.case(name)
    options = dict(c["options"]) if tiles is None else dict(c["options"], FR_LOOP_TILES=tiles)
    plan = plan_of(sim, trees[name], c["n_rows"], options, c["n_in"])
    s = plan["stream"]
    L.check_stream_object(s, c)
    assert plan["feedback"] and s["rings"] == plan["rings"]
    if tiles is None:
        with Renderer(sim, options=options) as r:                    # fr_stream_begin builds the tables (the simulator launches nothing)
            synth.install(r, trees[name])
            r.stream_begin(c["n_rows"])
            with pytest.raises(RenderError):
                r.stream_block_rows(0, [synth.time_ramp(0, 8)] * len(s["input_slots"]))
            r.fill_buffer(c["n_rows"], 0, 16, [synth.time_ramp(0, 16)] * c["n_in"])


def test_the_strides(sim, clean_env, trees):
    want = {"comb_1_2x128": 1, "comb_5_2x128": 5, "comb_63_2x256": 63, "taps_2_3": 1, "taps_6_9": 3, "taps_3_441": 3}
    for name, stride in want.items():
        c = L.case(name)
        s = plan_of(sim, trees[name], c["n_rows"], c["options"])["stream"]
        assert s["loop_programs"] == [stride, stride] and s["programs_per_voice"] == [1, 1], (name, s)


def test_a_tap_behind_a_loop_follows_the_loop_s_voice(sim, clean_env, trees):
    """Per voice, in the order they run: the loop (stride 5), then the tap that reads its ring 2 frames back (stride 0)."""
    c = L.case("tap_behind_loop")
    s = plan_of(sim, trees[c["name"]], c["n_rows"], c["options"])["stream"]
    assert s["programs_per_voice"] == [2, 2] and s["loop_programs"] == [5, 0, 5, 0] and s["bus_programs"] == 0, s
    assert s["min_ring_delay"] == 2


def test_bus_loops_sit_in_the_bus_segment(sim, clean_env, trees):
    for name, strides in (("bus_echo_32", [32]), ("summed_one_poles", [1])):
        c = L.case(name)
        s = plan_of(sim, trees[name], c["n_rows"], c["options"])["stream"]
        assert sum(s["programs_per_voice"]) == 0 and s["bus_programs"] == 1 and s["loop_programs"] == strides, (name, s)
    c = L.case("bus_one_pole_3x128_2")
    s = plan_of(sim, trees[c["name"]], c["n_rows"], c["options"])["stream"]
    assert sum(s["programs_per_voice"]) == 1 and s["bus_programs"] == 1 and s["loop_programs"] == [1, 1], s
    # without FR_STREAM_BUS the loops do not stand in for it
    for name in ("bus_echo_32", "summed_one_poles", "bus_one_pole_3x128_2"):
        c = L.case(name)
        s = plan_of(sim, trees[name], c["n_rows"], L.OPTION)["stream"]
        assert s["servable"] is False and "mix bus" in s["reason"], (name, s)


def test_a_loop_of_a_block_or_more_keeps_its_kernel(sim, clean_env):
    tree = L.comb_tree(4, 256, 64)
    a = plan_of(sim, tree, 4, L.PROGRAMS)["stream"]
    b = plan_of(sim, tree, 4, L.OPTION)["stream"]
    assert a["servable"] is True and not any(k in a for k in NEW_KEYS)
    assert {k: v for k, v in b.items() if k not in NEW_KEYS} == a
    assert b["loop_programs"] == [0] * 4 and b["kernel"] != L.NEW_KERNEL and (b["loop_loads"], b["loop_stores"]) == (L.LOOP_LOADS, L.LOOP_STORES)


@pytest.mark.parametrize("name", [c[0] for c in L.REFUSED])
def test_refused_with_the_option(sim, clean_env, trees, name):
    _, _, n_rows, options, why = K.case(L.REFUSED, name)
    s = plan_of(sim, trees[name], n_rows, options)["stream"]
    assert s["servable"] is False and why in s["reason"], s
    assert s["kernel"] != L.NEW_KERNEL and s["bus_programs"] == 0 and sum(s["programs_per_voice"]) == 0
    with Renderer(sim, options=options) as r:
        synth.install(r, trees[name])
        with pytest.raises(RenderError) as ei:
            r.stream_begin(n_rows)
        assert ei.value.status == FR_ERR_UNSUPPORTED and why in str(ei.value)
        r.fill_buffer(n_rows, 0, 16, [synth.time_ramp(0, 16)])


@pytest.mark.parametrize("off", [None, "0"])
@pytest.mark.parametrize("name", [c["name"] for c in L.SERVABLE])
def test_without_the_option_every_case_is_refused_as_before(sim, clean_env, trees, name, off):
    """Today's reason, with every other option of the case still on: a short read of a program's ring."""
    c = L.case(name)
    options = without(c["options"]) if off is None else dict(c["options"], FR_STREAM_LOOPS=off)
    s = plan_of(sim, trees[name], c["n_rows"], options, c["n_in"])["stream"]
    assert s["servable"] is False and s["kernel"] != L.NEW_KERNEL, s
    assert "frames back; a streamed block needs delays of at least 64 frames" in s["reason"] and s["reason"].startswith("a program's ring is read "), s
    if off is None:
        assert not any(k in s for k in NEW_KEYS)
        with Renderer(sim, options=options) as r:
            assert "FR_STREAM_LOOPS" not in r.options()
            synth.install(r, trees[name])
            with pytest.raises(RenderError) as ei:
                r.stream_begin(c["n_rows"])
            assert ei.value.status == FR_ERR_UNSUPPORTED and s["reason"] in str(ei.value)


def test_the_older_refusals_keep_their_text(sim, clean_env):
    for table, names, base in ((K.REFUSED, ("comb_63", "comb_32", "base_delay_32", "mix_row", "chorus", "small_voices"), L.PROGRAMS),
                               (B.REFUSED, ("bus_comb_32", "chorus"), B.OPTION)):
        for name in names:
            entry = K.case(table, name)
            tree, n_rows, why = entry[1](), entry[-2], entry[-1]               # (voices = output rows in K.REFUSED)
            a = plan_of(sim, tree, n_rows, base)["stream"]
            assert a["servable"] is False and why in a["reason"], (name, a)
            b = plan_of(sim, tree, n_rows, dict(base, FR_STREAM_LOOPS="1"))["stream"]
            if name in ("comb_63", "comb_32", "bus_comb_32"):          # what the option is for
                assert b["servable"] is True and b["kernel"] == L.NEW_KERNEL, (name, b)
            else:
                assert b["servable"] is False and b["reason"] == a["reason"], (name, b)


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_STREAM_LOOPS" not in r.options()
    with Renderer(sim, options=L.OPTION) as r:
        assert r.options()["FR_STREAM_LOOPS"] == {"value": "1", "source": "option"}
    clean_env.setenv("FR_STREAM_LOOPS", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_STREAM_LOOPS"] == {"value": "1", "source": "env"}
        assert "FR_STREAM_PROGRAMS" not in r.options()
    with Renderer(sim, options={"FR_STREAM_LOOPS": "0"}) as r:         # the option beats the environment
        assert r.options()["FR_STREAM_LOOPS"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_STREAM_LOOPS", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_STREAM_LOOPS": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_STREAM_LOOPS", bad)                       # the environment is read as strictly
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


def test_inert_without_stream_programs(sim, clean_env, trees):
    tree = trees["comb_5_2x128"]
    assert "stream" not in plan_of(sim, tree, 2, {"FR_STREAM_LOOPS": "1"})
    with Renderer(sim, options={"FR_STREAM_LOOPS": "1"}) as r:
        synth.install(r, tree)
        with pytest.raises(RenderError) as ei:
            r.stream_begin(2)
        assert ei.value.status == FR_ERR_UNSUPPORTED and "block streaming needs a plan that is one voice bank" in str(ei.value)
