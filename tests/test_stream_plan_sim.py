"""FR_STREAM_PROGRAMS on the CPU: the serving rule of block streaming (csrc/streamplan.hpp) through the engine's own host
code in the host-logic simulator.  With the option on, fr_plan_json carries "stream" after any ordinary call: whether one
resident launch can serve the plan, why not, and how the programs are dealt to the voices.  The simulator has no resident
launches (fr_stream_block needs the device): the kernel itself is tests/test_hip_stream_programs.py."""
import pytest

import sim_tools
import stream_cases as K
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, FR_ERR_UNSUPPORTED, RenderError, Renderer


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def stream_of(sim, tree, V, options=K.OPTION, **kw):
    with Renderer(sim, options=options, **kw) as r:
        synth.install(r, tree)
        r.fill_buffer(V, 0, 64, [synth.time_ramp(0, 64)])
        return r.plan()


@pytest.mark.parametrize("name", [c[0] for c in K.SERVABLE])
def test_servable(sim, clean_env, name):
    _, build, V, per_voice, min_delay = K.case(K.SERVABLE, name)
    tree = build()
    plan = stream_of(sim, tree, V)
    s = plan["stream"]
    assert s["servable"] is True and s["reason"] == "", s
    assert s["voices"] == V
    assert s["programs_per_voice"] == [per_voice] * V
    assert s["rings"] == plan["rings"]
    # chunks: halved from whole voices down to 128 partials while voices * chunks fits the kernel's 256 workgroups
    P = plan["banks"][0]["partials"]
    chunks = 1
    while P // (2 * chunks) >= 128 and V * 2 * chunks <= 256 and chunks < 256:
        chunks *= 2
    assert s["chunks"] == chunks
    assert s["min_ring_delay"] == min_delay


@pytest.mark.parametrize("name", [c[0] for c in K.REFUSED])
def test_refused(sim, clean_env, name):
    _, build, V, why = K.case(K.REFUSED, name)
    tree = build()
    s = stream_of(sim, tree, V)["stream"]
    assert s["servable"] is False and why in s["reason"], s
    assert s["programs_per_voice"] == [] or sum(s["programs_per_voice"]) == 0
    # fr_stream_begin refuses the same plan with the same reason, and the renderer stays usable
    with Renderer(sim, options=K.OPTION) as r:
        synth.install(r, tree)
        with pytest.raises(RenderError) as ei:
            r.stream_begin(V)
        assert ei.value.status == FR_ERR_UNSUPPORTED and why in str(ei.value)
        r.fill_buffer(V, 0, 16, [synth.time_ramp(0, 16)])


def test_pull_mode_is_refused_and_an_inert_track_history_is_not(sim, clean_env):
    s = stream_of(sim, synth.effects_tree(2, 128), 2, mode="pull")["stream"]
    assert s["servable"] is False and "FR_MODE_PULL" in s["reason"]
    s = stream_of(sim, synth.effects_tree(2, 128), 2, options={"FR_STREAM_PROGRAMS": "1", "FR_TRACK_HISTORY": "64"})["stream"]
    assert s["servable"] is True          # (no track slots declared: the history is inert)


def test_a_bare_bank_is_servable_without_programs(sim, clean_env):
    s = stream_of(sim, synth.additive_tree(3, 256), 3)["stream"]
    assert s["servable"] is True and s["programs_per_voice"] == [0, 0, 0] and s["rings"] == 0 and s["min_ring_delay"] == 0


def test_option_off_changes_nothing(sim, clean_env):
    plan = stream_of(sim, synth.effects_tree(4, 256), 4, options=None)
    assert "stream" not in plan
    plan = stream_of(sim, synth.effects_tree(4, 256), 4, options={"FR_STREAM_PROGRAMS": "0"})
    assert "stream" not in plan
    with Renderer(sim) as r:
        synth.install(r, synth.effects_tree(4, 256))
        with pytest.raises(RenderError) as ei:
            r.stream_begin(4)
        assert ei.value.status == FR_ERR_UNSUPPORTED
        assert "block streaming needs a plan that is one voice bank" in str(ei.value)


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_STREAM_PROGRAMS" not in r.options()
    with Renderer(sim, options=K.OPTION) as r:
        assert r.options()["FR_STREAM_PROGRAMS"] == {"value": "1", "source": "option"}
    clean_env.setenv("FR_STREAM_PROGRAMS", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_STREAM_PROGRAMS"] == {"value": "1", "source": "env"}
    with Renderer(sim, options={"FR_STREAM_PROGRAMS": "0"}) as r:      # the option beats the environment
        assert r.options()["FR_STREAM_PROGRAMS"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_STREAM_PROGRAMS", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_STREAM_PROGRAMS": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_STREAM_PROGRAMS", bad)                    # the environment is read as strictly
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


def test_begin_of_a_servable_plan_builds_its_tables_without_a_launch(sim, clean_env):
    """fr_stream_begin does not launch: on the simulator, which has no resident launches, it succeeds; the first block would
    launch and is refused with a device error, after which the renderer renders on."""
    with Renderer(sim, options=K.OPTION) as r:
        synth.install(r, synth.effects_tree(2, 128))
        r.stream_begin(2)
        with pytest.raises(RenderError):
            r.stream_block(0, synth.time_ramp(0, 8))
        r.fill_buffer(2, 0, 16, [synth.time_ramp(0, 16)])
