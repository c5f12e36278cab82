"""FR_STREAM_INPUTS on the CPU: the serving rule of block streaming with control rows (csrc/streamplan.hpp) through the
engine's own host code in the host-logic simulator, and the patches themselves against the oracle.  With FR_STREAM_PROGRAMS
and FR_STREAM_INPUTS on, fr_plan_json's "stream" lists the input slots whose rows a block brings ("input_slots", slot 0
first) and names the kernel that takes them.  The simulator has no resident launches: the kernel itself is
tests/test_hip_stream_inputs.py, the rows' bookkeeping tests/test_stream_rows_host.py."""
import numpy as np
import pytest

import sim_tools
import stream_bus_cases as B
import stream_cases as K
import stream_input_cases as I
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, FR_ERR_UNSUPPORTED, RenderError, Renderer


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def plan_of(sim, tree, n_rows, options):
    with Renderer(sim, options=options) as r:
        synth.install(r, tree)
        r.fill_buffer(n_rows, 0, 64, [synth.time_ramp(0, 64)])
        return r.plan()


@pytest.mark.parametrize("name", [c[0] for c in I.SERVABLE])
def test_servable_with_the_option(sim, clean_env, name):
    _, build, V, n_rows, slots, per_voice, bus, wgs = I.case(I.SERVABLE, name)
    plan = plan_of(sim, build(), n_rows, I.OPTION)
    s = plan["stream"]
    assert s["servable"] is True and s["reason"] == "", s
    assert s["input_slots"] == slots
    assert s["voices"] == V and s["voices"] * s["chunks"] == wgs and len(plan["banks"]) == 1
    assert s["programs_per_voice"] == per_voice and s["bus_programs"] == bus
    assert s["kernel"] == I.NEW_KERNEL
    with Renderer(sim, options=I.OPTION) as r:                     # fr_stream_begin builds the tables (the simulator launches nothing)
        synth.install(r, build())
        r.stream_begin(n_rows)
        with pytest.raises(RenderError):
            r.stream_block_rows(0, [synth.time_ramp(0, 8)] * len(slots))
        r.fill_buffer(n_rows, 0, 16, [synth.time_ramp(0, 16)])


@pytest.mark.parametrize("name", [c[0] for c in I.REFUSED])
def test_refused_with_the_option(sim, clean_env, name):
    _, build, V, n_rows, why = I.case(I.REFUSED, name)
    tree = build()
    s = plan_of(sim, tree, n_rows, I.OPTION)["stream"]
    assert s["servable"] is False and why in s["reason"], s
    assert s["kernel"] != I.NEW_KERNEL
    with Renderer(sim, options=I.OPTION) as r:
        synth.install(r, tree)
        with pytest.raises(RenderError) as ei:
            r.stream_begin(n_rows)
        assert ei.value.status == FR_ERR_UNSUPPORTED and why in str(ei.value)
        r.fill_buffer(n_rows, 0, 16, [synth.time_ramp(0, 16)])


@pytest.mark.parametrize("off", [None, "0"])
@pytest.mark.parametrize("name", [c[0] for c in I.SERVABLE] + ["nine_slots"])
def test_without_the_option_every_case_is_refused_as_before(sim, clean_env, name, off):
    c = I.case(I.SERVABLE + I.REFUSED, name)
    build, n_rows = c[1], c[3]
    tree = build()
    options = dict(I.OFF) if off is None else dict(I.OFF, FR_STREAM_INPUTS=off)
    s = plan_of(sim, tree, n_rows, options)["stream"]
    assert s["servable"] is False and s["reason"].startswith("a program reads input slot ") and s["reason"].endswith("; " + I.OLD_REASON), s
    assert s["input_slots"] == [0] and s["kernel"] != I.NEW_KERNEL
    with Renderer(sim, options=options) as r:
        synth.install(r, tree)
        with pytest.raises(RenderError) as ei:
            r.stream_begin(n_rows)
        assert ei.value.status == FR_ERR_UNSUPPORTED and I.OLD_REASON in str(ei.value)


def test_a_delayed_input_keeps_its_reason_either_way(sim, clean_env):
    _, build, V, n_rows, why = I.case(I.REFUSED, "delayed_input")
    for options in (I.OFF, I.OPTION):
        s = plan_of(sim, build(), n_rows, options)["stream"]
        assert s["servable"] is False and why in s["reason"] and "does not serve yet" in s["reason"], s


@pytest.mark.parametrize("name", [c[0] for c in K.SERVABLE])
def test_plans_of_stream_cases_read_slot_0_only(sim, clean_env, name):
    _, build, V, per_voice, min_delay = K.case(K.SERVABLE, name)
    tree = build()
    a = plan_of(sim, tree, V, B.OPTION)["stream"]
    b = plan_of(sim, tree, V, I.OPTION)["stream"]
    assert b["input_slots"] == [0] and b["kernel"] == a["kernel"] != I.NEW_KERNEL
    assert a == b and b["programs_per_voice"] == [per_voice] * V


@pytest.mark.parametrize("name", [c[0] for c in B.SERVABLE])
def test_plans_of_stream_bus_cases_read_slot_0_only(sim, clean_env, name):
    _, build, V, n_rows, per_voice, bus = B.case(B.SERVABLE, name)
    tree = build()
    a = plan_of(sim, tree, n_rows, B.OPTION)["stream"]
    b = plan_of(sim, tree, n_rows, I.OPTION)["stream"]
    assert b["input_slots"] == [0] and b["kernel"] == a["kernel"] != I.NEW_KERNEL
    assert a == b and b["programs_per_voice"] == per_voice and b["bus_programs"] == bus


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_STREAM_INPUTS" not in r.options()
    with Renderer(sim, options=I.OPTION) as r:
        assert r.options()["FR_STREAM_INPUTS"] == {"value": "1", "source": "option"}
    clean_env.setenv("FR_STREAM_INPUTS", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_STREAM_INPUTS"] == {"value": "1", "source": "env"}
    with Renderer(sim, options={"FR_STREAM_INPUTS": "0"}) as r:        # the option beats the environment
        assert r.options()["FR_STREAM_INPUTS"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_STREAM_INPUTS", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_STREAM_INPUTS": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_STREAM_INPUTS", bad)                      # the environment is read as strictly
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


def test_inert_without_stream_programs(sim, clean_env):
    tree = I.gain_tree(2, 128)
    assert "stream" not in plan_of(sim, tree, 2, {"FR_STREAM_INPUTS": "1"})
    with Renderer(sim, options={"FR_STREAM_INPUTS": "1"}) as r:
        synth.install(r, tree)
        with pytest.raises(RenderError) as ei:
            r.stream_begin(2)
        assert ei.value.status == FR_ERR_UNSUPPORTED and "block streaming needs a plan that is one voice bank" in str(ei.value)


def test_the_binding_resolves_the_entry_point(sim, oracle_lib):
    assert sim.has_stream_rows is True and oracle_lib.has_stream_rows is False
    with Renderer(oracle_lib) as r:
        with pytest.raises(RenderError) as ei:
            r.stream_block_rows(0, [synth.time_ramp(0, 8)])
        assert ei.value.status == FR_ERR_UNSUPPORTED
    with Renderer(sim) as r:
        with pytest.raises(RenderError) as ei:                         # no stream is open
            r.stream_block_rows(0, [synth.time_ramp(0, 8)])
        assert ei.value.status == FR_ERR_INVALID_ARG


@pytest.mark.parametrize("semantics", ["reference", "sparkle"])
@pytest.mark.parametrize("name", [c[0] for c in I.SERVABLE])
def test_the_patches_against_the_oracle(sim, oracle_lib, clean_env, name, semantics):
    """fr_fill_buffer of the simulator (options on: they change no ordinary call) against the oracle, four blocks with
    control rows of every kind, the first block a seek."""
    _, build, V, n_rows, slots, _, _, _ = I.case(I.SERVABLE, name)
    tree = build()
    rng = np.random.default_rng(len(name))
    blocks = I.block_inputs(rng, [(300, 4 * 64)], len(slots))[:4]
    with Renderer(sim, semantics=semantics, options=I.OPTION) as r, Renderer(oracle_lib, semantics=semantics) as ref:
        synth.install(r, tree)
        synth.install(ref, tree)
        loud = 0.0
        for k, (idx, T, rows) in enumerate(blocks):
            a = r.fill_buffer(n_rows, idx, idx + T, rows)
            b = ref.fill_buffer(n_rows, idx, idx + T, rows)
            assert K.same_bits(a, b), f"{name} block {k} at frame {idx}: " + K.first_diff(a, b)
            loud = max(loud, float(np.nanmax(np.abs(np.where(np.isfinite(a), a, 0)))))
        assert loud > 0.01
