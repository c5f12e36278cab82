"""FR_STREAM_BANKS on the CPU: the serving rule of block streaming for plans of several banks (csrc/streamplan.hpp) through
the engine's own host code in the host-logic simulator.  With FR_STREAM_PROGRAMS and FR_STREAM_BANKS on, fr_plan_json's
"stream" lists the banks of the launch ("banks": voices, partials, chunks, to_ring), its workgroups and the limit they were
dealt under, and names the kernel.  The simulator has no resident launches: the kernel itself is
tests/test_hip_stream_banks.py, the chunk rule on its own tests/test_stream_banks_host.py."""
import pytest

import sim_tools
import stream_banks_cases as M
import stream_bus_cases as B
import stream_cases as K
import stream_input_cases as I
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, FR_ERR_UNSUPPORTED, RenderError, Renderer

NEW_KEYS = ("banks", "workgroups", "max_workgroups")


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture(scope="module")
def trees():
    """Every case's graph, built once."""
    return {c[0]: c[1]() for c in M.SERVABLE + M.REFUSED}


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def plan_of(sim, tree, n_rows, options):
    with Renderer(sim, options=options) as r:
        synth.install(r, tree)
        r.fill_buffer(n_rows, 0, 64, [synth.time_ramp(0, 64)])
        assert ("FR_STREAM_BANKS" in r.options()) == ("FR_STREAM_BANKS" in options)
        return r.plan()


@pytest.mark.parametrize("name", [c[0] for c in M.SERVABLE])
def test_servable_with_the_option(sim, clean_env, trees, name):
    _, _, n_rows, options, banks, per_voice, bus, slots = M.case(M.SERVABLE, name)
    plan = plan_of(sim, trees[name], n_rows, options)
    s = plan["stream"]
    got = M.check_stream_object(s, banks, per_voice, bus, slots)
    assert s["max_workgroups"] == 256                                # (a device the simulator does not have: the kernel's limit)
    assert len(plan["banks"]) == len(got) >= 2
    assert s["rings"] == plan["rings"]
    with Renderer(sim, options=options) as r:                        # fr_stream_begin builds the tables (the simulator launches nothing)
        synth.install(r, trees[name])
        r.stream_begin(n_rows)
        with pytest.raises(RenderError):
            r.stream_block_rows(0, [synth.time_ramp(0, 8)] * len(slots))
        r.fill_buffer(n_rows, 0, 16, [synth.time_ramp(0, 16)])


def test_the_chunked_and_the_unchunked_bank(sim, clean_env, trees):
    s = plan_of(sim, trees["rows_two_sizes"], 4, M.OPTION)["stream"]
    by_size = {b["partials"]: b for b in s["banks"]}
    assert by_size[128]["chunks"] == 1 and by_size[1024]["chunks"] == 8 and s["workgroups"] == 2 + 16 and s["chunks"] == 8
    s = plan_of(sim, trees["chord_bus"], 2, M.OPTION)["stream"]
    assert {b["partials"]: b["chunks"] for b in s["banks"]} == {1024: 8, 256: 2, 128: 1} and s["workgroups"] == 16 + 6 + 4


@pytest.mark.parametrize("name", [c[0] for c in M.REFUSED])
def test_refused_with_the_option(sim, clean_env, trees, name):
    _, _, n_rows, n_banks, why = M.case(M.REFUSED, name)
    plan = plan_of(sim, trees[name], n_rows, M.OPTION)
    s = plan["stream"]
    assert len(plan["banks"]) == n_banks
    assert s["servable"] is False and why in s["reason"], s
    assert s["kernel"] != M.NEW_KERNEL and s["bus_programs"] == 0 and sum(s["programs_per_voice"]) == 0
    with Renderer(sim, options=M.OPTION) as r:
        synth.install(r, trees[name])
        with pytest.raises(RenderError) as ei:
            r.stream_begin(n_rows)
        assert ei.value.status == FR_ERR_UNSUPPORTED and why in str(ei.value)
        r.fill_buffer(n_rows, 0, 16, [synth.time_ramp(0, 16)])


@pytest.mark.parametrize("off", [None, "0"])
@pytest.mark.parametrize("name", [c[0] for c in M.SERVABLE + M.REFUSED])
def test_without_the_option_every_case_is_refused_as_before(sim, clean_env, trees, name, off):
    n_rows = M.case(M.SERVABLE + M.REFUSED, name)[2]
    options = dict(M.OFF) if off is None else dict(M.OFF, FR_STREAM_BANKS=off)
    plan = plan_of(sim, trees[name], n_rows, options)
    s = plan["stream"]
    assert s["servable"] is False and s["reason"] == M.old_reason(len(plan["banks"])) and len(plan["banks"]) >= 2, s
    assert s["kernel"] != M.NEW_KERNEL and s["voices"] == 0
    if off is None:
        assert not any(k in s for k in NEW_KEYS)
        with Renderer(sim, options=options) as r:
            assert "FR_STREAM_BANKS" not in r.options()
            synth.install(r, trees[name])
            with pytest.raises(RenderError) as ei:
                r.stream_begin(n_rows)
            # (a plan with programs or rings: the rule's text; one without: fr_stream_begin's own, as it has always been)
            assert ei.value.status == FR_ERR_UNSUPPORTED and f"{len(plan['banks'])} bank launches" in str(ei.value)
            assert ("block streaming needs a plan with one voice bank" in str(ei.value)) or ("block streaming needs a plan that is one voice bank" in str(ei.value))


@pytest.mark.parametrize("table,name", [("K", c[0]) for c in K.SERVABLE if c[2] <= 16] + [("B", c[0]) for c in B.SERVABLE if c[2] <= 16] +
                         [("I", c[0]) for c in I.SERVABLE])
def test_one_bank_is_served_as_before(sim, clean_env, table, name):
    """A single-bank plan reports the same "stream" object with the option on as with it off, apart from the new keys; its one
    bank is dealt what the plan's scalar fields say."""
    if table == "K":
        _, build, n_rows, _, _ = K.case(K.SERVABLE, name)
    elif table == "B":
        _, build, _, n_rows, _, _ = B.case(B.SERVABLE, name)
    else:
        _, build, _, n_rows = I.case(I.SERVABLE, name)[:4]
    tree = build()
    a = plan_of(sim, tree, n_rows, M.OFF)["stream"]
    b = plan_of(sim, tree, n_rows, M.OPTION)["stream"]
    assert a["servable"] is True and not any(k in a for k in NEW_KEYS)
    assert {k: v for k, v in b.items() if k not in NEW_KEYS} == a
    assert b["kernel"] != M.NEW_KERNEL and len(b["banks"]) == 1
    assert b["banks"][0]["voices"] == a["voices"] and b["banks"][0]["chunks"] == a["chunks"] and b["workgroups"] == a["voices"] * a["chunks"]


def test_single_bank_refusals_keep_their_text(sim, clean_env):
    for table, names in ((K.REFUSED, ("comb_63", "mix_row", "small_voices", "more_voices_than_cus")),):
        for name in names:
            _, build, V, why = K.case(table, name)
            tree = build()
            a = plan_of(sim, tree, V, M.PROGRAMS)["stream"]
            b = plan_of(sim, tree, V, dict(M.PROGRAMS, FR_STREAM_BANKS="1"))["stream"]
            assert a["servable"] is False and why in a["reason"] and b["reason"] == a["reason"]


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_STREAM_BANKS" not in r.options()
    with Renderer(sim, options=M.OPTION) as r:
        assert r.options()["FR_STREAM_BANKS"] == {"value": "1", "source": "option"}
    clean_env.setenv("FR_STREAM_BANKS", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_STREAM_BANKS"] == {"value": "1", "source": "env"}
        assert "FR_STREAM_PROGRAMS" not in r.options()
    with Renderer(sim, options={"FR_STREAM_BANKS": "0"}) as r:         # the option beats the environment
        assert r.options()["FR_STREAM_BANKS"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_STREAM_BANKS", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_STREAM_BANKS": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_STREAM_BANKS", bad)                       # the environment is read as strictly
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


def test_inert_without_stream_programs(sim, clean_env, trees):
    tree = trees["rows_two_sizes"]
    assert "stream" not in plan_of(sim, tree, 4, {"FR_STREAM_BANKS": "1"})
    with Renderer(sim, options={"FR_STREAM_BANKS": "1"}) as r:
        synth.install(r, tree)
        with pytest.raises(RenderError) as ei:
            r.stream_begin(4)
        assert ei.value.status == FR_ERR_UNSUPPORTED and "block streaming needs a plan that is one voice bank (this one: 2 bank launches" in str(ei.value)


def test_the_bus_and_the_rows_still_need_their_options(sim, clean_env, trees):
    """FR_STREAM_BANKS composes with the two others, it does not stand in for them."""
    s = plan_of(sim, trees["chord_bus"], 2, dict(M.PROGRAMS, FR_STREAM_BANKS="1"))["stream"]
    assert s["servable"] is False and "mix bus" in s["reason"]
    s = plan_of(sim, trees["chord_gated"], 2, dict(B.OPTION, FR_STREAM_BANKS="1"))["stream"]
    assert s["servable"] is False and s["reason"].endswith("; " + I.OLD_REASON)
    s = plan_of(sim, trees["dry_and_enveloped"], 4, dict(M.PROGRAMS, FR_STREAM_BANKS="1"))["stream"]
    assert s["servable"] is True and s["kernel"] == M.NEW_KERNEL
