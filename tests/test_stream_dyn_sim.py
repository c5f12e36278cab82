"""FR_STREAM_DYN on the CPU: the serving rule of block streaming for Delays by a signal amount (csrc/streamplan.hpp) through the
engine's own host code in the host-logic simulator.  With FR_STREAM_PROGRAMS and FR_STREAM_DYN on, a program that delays a voice
by a signal amount is served -- fr_plan_json's "stream" counts the ops ("dyn_reads", "dyn_steps"), gives the deepest ring read
("lookback") and names the kernel --; what stays refused says so; with the option absent or 0 every answer is what it was.  The
simulator has no resident launches: the kernel itself is tests/test_hip_stream_dyn.py; the rule on hand-built plans, the launch
rule and a host model of the two ops are tests/test_stream_dyn_host.py."""
import numpy as np
import pytest

import sim_tools
import stream_banks_cases as M
import stream_bus_cases as B
import stream_cases as K
import stream_dyn_cases as D
import stream_general_cases as G
import stream_input_cases as I
import stream_loop_cases as L
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, FR_ERR_UNSUPPORTED, RenderError, Renderer


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture(scope="module")
def trees():
    """Every case's graph, built once."""
    t = {c["name"]: c["build"]() for c in D.SERVABLE}
    t.update({c[0]: c[1]() for c in D.REFUSED})
    return t


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN", "FR_LOOP_TILES",
              "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def plan_of(sim, tree, n_rows, options, n_in=1):
    with Renderer(sim, options=options) as r:
        synth.install(r, tree)
        r.fill_buffer(n_rows, 0, 64, [synth.time_ramp(0, 64)] + [np.ones(64, np.float32)] * (n_in - 1))
        assert ("FR_STREAM_DYN" in r.options()) == ("FR_STREAM_DYN" in options)
        return r.plan()


def without(options):
    return {k: v for k, v in options.items() if k != "FR_STREAM_DYN"}


@pytest.mark.parametrize("name", [c["name"] for c in D.SERVABLE])
def test_servable_with_the_option(sim, clean_env, trees, name):
    c = D.case(name)
    s = plan_of(sim, trees[name], c["n_rows"], c["options"], c["n_in"])["stream"]
    D.check_stream_object(s, c)
    with Renderer(sim, options=c["options"]) as r:                   # fr_stream_begin builds the tables (the simulator launches nothing)
        synth.install(r, trees[name])
        r.stream_begin(c["n_rows"])
        with pytest.raises(RenderError):
            r.stream_block_rows(0, [synth.time_ramp(0, 8)] * len(s["input_slots"]))
        r.fill_buffer(c["n_rows"], 0, 16, [synth.time_ramp(0, 16)] * c["n_in"])


def test_the_bound_sizes_the_lookback(sim, clean_env, trees):
    """The chorus of 400..700 frames: the deepest ring read is the planner's bound, whatever the block length."""
    s = plan_of(sim, trees["chorus_2x128"], 2, D.OPTION)["stream"]
    assert 700 <= s["lookback"] < 1024 and s["min_ring_delay"] == 0 and s["programs_per_voice"] == [1, 1], s
    s = plan_of(sim, trees["chorus_taps"], 2, D.OPTION)["stream"]     # the taps' rings are programs' rings: 100 frames is their shortest read
    assert s["min_ring_delay"] == 100 and s["lookback"] >= 200, s


@pytest.mark.parametrize("name", [c[0] for c in D.REFUSED])
def test_refused_with_the_option(sim, clean_env, trees, name):
    _, _, n_rows, options, n_in, why = K.case(D.REFUSED, name)
    s = plan_of(sim, trees[name], n_rows, options, n_in)["stream"]
    assert s["servable"] is False and all(w in s["reason"] for w in why), s
    assert s["kernel"] != D.NEW_KERNEL and all(k in s for k in D.NEW_KEYS)
    assert "(a Delay by a signal amount)" not in s["reason"]           # the text names only what is still refused
    with Renderer(sim, options=options) as r:
        synth.install(r, trees[name])
        r.fill_buffer(n_rows, 0, 64, [synth.time_ramp(0, 64)] + [np.ones(64, np.float32)] * (n_in - 1))
        with pytest.raises(RenderError) as ei:
            r.stream_begin(n_rows)
        assert ei.value.status == FR_ERR_UNSUPPORTED and all(w in str(ei.value) for w in why)
        r.fill_buffer(n_rows, 64, 80, [synth.time_ramp(64, 80)] + [np.ones(16, np.float32)] * (n_in - 1))


@pytest.mark.parametrize("name,reason", [("chorus_2x128", D.OLD_REASON), ("knob", D.OLD_REASON), ("beside_loop", D.OLD_REASON)])
@pytest.mark.parametrize("off", [None, "0"])
def test_without_the_option_the_reason_is_today_s(sim, clean_env, trees, name, reason, off):
    c = D.case(name)
    options = without(c["options"]) if off is None else dict(c["options"], FR_STREAM_DYN=off)
    s = plan_of(sim, trees[name], c["n_rows"], options, c["n_in"])["stream"]
    assert s["servable"] is False and s["reason"] == reason and s["kernel"] != D.NEW_KERNEL, s
    assert not any(k in s for k in D.NEW_KEYS)
    with Renderer(sim, options=options) as r:
        assert ("FR_STREAM_DYN" in r.options()) == (off is not None)
        synth.install(r, trees[name])
        with pytest.raises(RenderError) as ei:
            r.stream_begin(c["n_rows"])
        assert ei.value.status == FR_ERR_UNSUPPORTED and reason in str(ei.value)


def _older_cases():
    """A prog, a bus, an in, a loops and a general plan of the existing case modules: (id, builder, rows, options, input rows)."""
    name, build, V, _, _ = K.case(K.SERVABLE, "effects_2x128")
    yield "prog/" + name, build, V, K.OPTION, 1
    name, build = B.SERVABLE[0][0], B.SERVABLE[0][1]
    yield "bus/" + name, build, B.SERVABLE[0][3], B.OPTION, 1
    name, build, _, n_rows, slots, _, _, _ = I.case(I.SERVABLE, "gain_2x128")
    yield "in/" + name, build, n_rows, I.OPTION, len(slots)
    c = L.case("comb_5_2x128")
    yield "loops/" + c["name"], c["build"], c["n_rows"], c["options"], c["n_in"]
    c = G.case("additive_2x100")
    yield "general/" + c["name"], c["build"], c["n_rows"], c["options"], c["n_in"]
    name, build, n_rows, options, _, _, _, slots = M.SERVABLE[0]
    yield "banks/" + name, build, n_rows, options, len(slots)


@pytest.mark.parametrize("case", list(_older_cases()), ids=lambda c: c[0])
def test_a_plan_without_a_signal_delay_keeps_its_stream_object(sim, clean_env, case):
    """With the option on: the object it has with the option off, key for key and in the same order, plus the new keys with no
    signal delay counted -- the kernel name included."""
    _, build, n_rows, options, n_in = case
    tree = build()
    a = plan_of(sim, tree, n_rows, options, n_in)["stream"]
    b = plan_of(sim, tree, n_rows, dict(options, FR_STREAM_DYN="1"), n_in)["stream"]
    assert a["servable"] is True and not any(k in a for k in D.NEW_KEYS), a
    stripped = {k: v for k, v in b.items() if k not in D.NEW_KEYS}
    assert stripped == a and list(stripped) == list(a)
    assert b["dyn_reads"] == 0 and b["dyn_steps"] == 0 and b["kernel"] != D.NEW_KERNEL, b


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_STREAM_DYN" not in r.options()
    with Renderer(sim, options=D.OPTION) as r:
        assert r.options()["FR_STREAM_DYN"] == {"value": "1", "source": "option"}
    clean_env.setenv("FR_STREAM_DYN", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_STREAM_DYN"] == {"value": "1", "source": "env"}
        assert "FR_STREAM_PROGRAMS" not in r.options()
    with Renderer(sim, options={"FR_STREAM_DYN": "0"}) as r:          # the option beats the environment
        assert r.options()["FR_STREAM_DYN"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_STREAM_DYN", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_STREAM_DYN": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_STREAM_DYN", bad)                        # the environment is read as strictly
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


def test_inert_without_stream_programs(sim, clean_env, trees):
    tree = trees["chorus_2x128"]
    assert "stream" not in plan_of(sim, tree, 2, {"FR_STREAM_DYN": "1"})
    said = []
    for options in ({"FR_STREAM_DYN": "1"}, {}):                      # the plain path's refusal, word for word what a renderer without options says
        with Renderer(sim, options=options) as r:
            synth.install(r, tree)
            with pytest.raises(RenderError) as ei:
                r.stream_begin(2)
            assert ei.value.status == FR_ERR_UNSUPPORTED and "block streaming needs a plan that is one voice bank" in str(ei.value)
            said.append(str(ei.value))
    assert said[0] == said[1]
