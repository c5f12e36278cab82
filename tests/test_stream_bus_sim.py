"""FR_STREAM_BUS on the CPU: the serving rule of block streaming with mix-bus programs (csrc/streamplan.hpp) through the
engine's own host code in the host-logic simulator.  With FR_STREAM_PROGRAMS and FR_STREAM_BUS on, fr_plan_json's "stream"
says how many programs follow each voice and how many run after the block's last voice ("bus_programs").  The simulator has
no resident launches: the kernel itself is tests/test_hip_stream_bus.py."""
import pytest

import sim_tools
import stream_bus_cases as B
import stream_cases as K
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, FR_ERR_UNSUPPORTED, RenderError, Renderer


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def plan_of(sim, tree, n_rows, options):
    with Renderer(sim, options=options) as r:
        synth.install(r, tree)
        r.fill_buffer(n_rows, 0, 64, [synth.time_ramp(0, 64)])
        return r.plan()


def one_launch_programs(plan):
    """The programs of the plan's one-launch form: the fused programs (a feedback plan: with its row copies), or the plan's
    only level."""
    return plan["fused_programs"] + plan["copy_programs"] if plan["fused_programs"] else plan["stage_programs"]


@pytest.mark.parametrize("name", [c[0] for c in B.SERVABLE])
def test_servable_with_the_bus(sim, clean_env, name):
    _, build, V, n_rows, per_voice, bus = B.case(B.SERVABLE, name)
    plan = plan_of(sim, build(), n_rows, B.OPTION)
    s = plan["stream"]
    assert s["servable"] is True and s["reason"] == "", s
    assert s["voices"] == V and plan["banks"][0]["to_ring"] is True and len(plan["banks"]) == 1
    assert s["programs_per_voice"] == per_voice
    assert s["bus_programs"] == bus
    assert sum(s["programs_per_voice"]) + s["bus_programs"] == one_launch_programs(plan)
    assert s["rings"] == plan["rings"]


@pytest.mark.parametrize("off", [None, "0"])
@pytest.mark.parametrize("name", [c[0] for c in B.SERVABLE])
def test_the_same_cases_are_refused_without_the_bus(sim, clean_env, name, off):
    _, build, V, n_rows, _, _ = B.case(B.SERVABLE, name)
    tree = build()
    options = dict(B.PROGRAMS) if off is None else dict(B.PROGRAMS, FR_STREAM_BUS=off)
    s = plan_of(sim, tree, n_rows, options)["stream"]
    assert s["servable"] is False and "mix bus" in s["reason"], s
    assert s["bus_programs"] == 0 and sum(s["programs_per_voice"]) == 0
    if off is None and V <= 8:      # fr_stream_begin refuses the same plan with the same reason, and the renderer stays usable
        with Renderer(sim, options=options) as r:
            synth.install(r, tree)
            with pytest.raises(RenderError) as ei:
                r.stream_begin(n_rows)
            assert ei.value.status == FR_ERR_UNSUPPORTED and "mix bus" in str(ei.value)
            r.fill_buffer(n_rows, 0, 16, [synth.time_ramp(0, 16)])


@pytest.mark.parametrize("name", [c[0] for c in B.REFUSED])
def test_still_refused_with_the_bus(sim, clean_env, name):
    _, build, V, n_rows, why = B.case(B.REFUSED, name)
    tree = build()
    s = plan_of(sim, tree, n_rows, B.OPTION)["stream"]
    assert s["servable"] is False and why in s["reason"], s
    assert s["bus_programs"] == 0 and sum(s["programs_per_voice"]) == 0
    with Renderer(sim, options=B.OPTION) as r:
        synth.install(r, tree)
        with pytest.raises(RenderError) as ei:
            r.stream_begin(n_rows)
        assert ei.value.status == FR_ERR_UNSUPPORTED and why in str(ei.value)
        r.fill_buffer(n_rows, 0, 16, [synth.time_ramp(0, 16)])


@pytest.mark.parametrize("name", [c[0] for c in K.SERVABLE])
def test_plans_without_a_bus_are_dealt_as_before(sim, clean_env, name):
    """What FR_STREAM_PROGRAMS serves alone has no bus program with the bus on, and the same programs per voice."""
    _, build, V, per_voice, min_delay = K.case(K.SERVABLE, name)
    tree = build()
    a = plan_of(sim, tree, V, B.PROGRAMS)["stream"]
    b = plan_of(sim, tree, V, B.OPTION)["stream"]
    assert a == b and b["bus_programs"] == 0 and b["programs_per_voice"] == [per_voice] * V and b["min_ring_delay"] == min_delay


@pytest.mark.parametrize("name", ["comb_63", "comb_32", "base_delay_32"])
def test_short_delays_behind_one_voice_stay_refused(sim, clean_env, name):
    _, build, V, why = K.case(K.REFUSED, name)
    s = plan_of(sim, build(), V, B.OPTION)["stream"]
    assert s["servable"] is False and why in s["reason"], s


def test_a_bus_of_bare_voices_is_no_bus(sim, clean_env):
    """A plain Sum2 of bare voices is folded into one larger voice by the matcher: served without the bus option."""
    g = synth.GraphArrays()
    p = synth.voice_params(2, 128, 1)
    x = synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(2, 128))
    g.edge(g.binop(synth.K_SUM2, x[:1], x[1:], 1), 0, 0, 0)
    s = plan_of(sim, g.finish(1), 1, B.PROGRAMS)["stream"]
    assert s["servable"] is True and s["voices"] == 1 and s["bus_programs"] == 0


def test_begin_of_a_bus_plan_builds_its_tables_without_a_launch(sim, clean_env):
    with Renderer(sim, options=B.OPTION) as r:
        synth.install(r, B.mixdown_tree(4, 128, 2))
        r.stream_begin(2)
        with pytest.raises(RenderError):
            r.stream_block(0, synth.time_ramp(0, 8))      # (the simulator has no resident launches)
        r.fill_buffer(2, 0, 16, [synth.time_ramp(0, 16)])


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_STREAM_BUS" not in r.options()
    with Renderer(sim, options=B.OPTION) as r:
        assert r.options()["FR_STREAM_BUS"] == {"value": "1", "source": "option"}
        assert r.options()["FR_STREAM_PROGRAMS"] == {"value": "1", "source": "option"}
    clean_env.setenv("FR_STREAM_BUS", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_STREAM_BUS"] == {"value": "1", "source": "env"}
        assert "FR_STREAM_PROGRAMS" not in r.options()
    with Renderer(sim, options={"FR_STREAM_BUS": "0"}) as r:          # the option beats the environment
        assert r.options()["FR_STREAM_BUS"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_STREAM_BUS", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_STREAM_BUS": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_STREAM_BUS", bad)                        # the environment is read as strictly
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG
    clean_env.delenv("FR_STREAM_BUS", raising=False)
    with pytest.raises(RenderError) as ei:                            # FR_STREAM_PROGRAMS keeps refusing "2"
        Renderer(sim, options={"FR_STREAM_PROGRAMS": "2", "FR_STREAM_BUS": "1"})
    assert ei.value.status == FR_ERR_INVALID_ARG


def test_inert_without_stream_programs(sim, clean_env):
    tree = B.mixdown_tree(2, 128, 1)
    plan = plan_of(sim, tree, 1, {"FR_STREAM_BUS": "1"})
    assert "stream" not in plan
    with Renderer(sim, options={"FR_STREAM_BUS": "1"}) as r:
        synth.install(r, tree)
        with pytest.raises(RenderError) as ei:
            r.stream_begin(1)
        assert ei.value.status == FR_ERR_UNSUPPORTED
        assert "block streaming needs a plan that is one voice bank" in str(ei.value)
