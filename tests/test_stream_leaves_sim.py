"""FR_STREAM_LEAVES on the CPU, through the engine's own host code in the host-logic simulator (tests/sim_tools.py).  The simulator
has no run-time compiler, so its plans never hold a compiled bank: what the rule makes of one is tests/test_stream_leaves_host.py's,
what the two leaf kernels compute tests/test_hip_stream_leaves.py's.

Covered here: the option's plumbing and strictness; fr_plan_json of three plans without a compiled bank -- unchanged with the option
unset or 0, and with 1 unchanged apart from "leaf_banks": []; the simulator's answer for the triangle patch, which is today's
sentence word for word with the option on or off; and, before anything runs on a GPU, the conditions on the inputs: the simulator's
fr_fill_buffer of every case of tests/stream_leaves_cases.py but the hostile one is at least 95 % finite and audible in every row."""
import numpy as np
import pytest

import sim_tools
import stream_cases as K
import stream_fx_cases as FX
import stream_leaves_cases as L
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, FR_ERR_UNSUPPORTED, RenderError, Renderer

STREAM_KEYS = ("FR_LOOP_DYN", "FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN",
               "FR_STREAM_HISTORY", "FR_STREAM_EFFECTS", "FR_STREAM_STORE", "FR_STREAM_TAPS", "FR_STREAM_SWEEP", "FR_STREAM_LEAVES", "FR_LOOP_TILES", "FR_STAGE_JIT")


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in STREAM_KEYS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_STREAM_LEAVES" not in r.options()
    for v in ("0", "1"):
        with Renderer(sim, options={"FR_STREAM_LEAVES": v}) as r:
            assert r.options()["FR_STREAM_LEAVES"] == {"value": v, "source": "option"}
    clean_env.setenv("FR_STREAM_LEAVES", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_STREAM_LEAVES"] == {"value": "1", "source": "env"}
    with Renderer(sim, options={"FR_STREAM_LEAVES": "0"}) as r:      # the option beats the environment
        assert r.options()["FR_STREAM_LEAVES"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_STREAM_LEAVES", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_STREAM_LEAVES": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_STREAM_LEAVES", bad)
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


def test_inert_without_stream_programs(sim):
    """FR_STREAM_LEAVES=1 alone: no "stream" object, as without it."""
    tree = K.comb_tree(2, 128, 100)
    with Renderer(sim, options={"FR_STREAM_LEAVES": "1"}) as r:
        synth.install(r, tree)
        r.fill_buffer(2, 0, 16, [np.arange(16, dtype=np.float32)])
        assert "stream" not in r.plan()


NO_COMPILED_BANK = [
    ("template_bank_with_envelope", lambda: synth.effects_tree(2, 128, taps=0), 2, 1, K.OPTION),
    ("voiceless_echo", lambda: FX.echo_tree(100), 1, 2, FX.INPUTS),
    ("general_voice", lambda: synth.additive_tree(2, 96), 2, 1, dict(K.OPTION, FR_STREAM_GENERAL="1")),
]


@pytest.mark.parametrize("name,build,n_rows,n_in,options", NO_COMPILED_BANK, ids=[c[0] for c in NO_COMPILED_BANK])
def test_plans_without_a_compiled_bank_are_unchanged(sim, name, build, n_rows, n_in, options):
    """fr_plan_json with the option unset and 0: the same, key for key; with 1 the stream object gains "leaf_banks": [] and
    everything else -- servable, the kernel, the reason -- stays."""
    tree = build()
    rows = [np.arange(16, dtype=np.float32)] * n_in
    plans = {}
    for key, extra in (("unset", {}), ("0", {"FR_STREAM_LEAVES": "0"}), ("1", {"FR_STREAM_LEAVES": "1"})):
        with Renderer(sim, options=dict(options, FR_STAGE_JIT="0", **extra)) as r:
            synth.install(r, tree)
            r.fill_buffer(n_rows, 0, 16, rows)
            plans[key] = {k: v for k, v in r.plan().items() if k not in ("build_ms", "lower_ms", "jit_compile_ms")}
    assert plans["unset"]["stream"]["servable"] is True, plans["unset"]["stream"]
    assert "leaf_banks" not in plans["unset"]["stream"]
    assert plans["unset"] == plans["0"]
    on = dict(plans["1"])
    stream = dict(on.pop("stream"))
    assert stream.pop("leaf_banks") == []
    off = dict(plans["unset"])
    assert stream == off.pop("stream") and on == off


@pytest.mark.parametrize("extra", [{}, {"FR_STREAM_LEAVES": "0"}, {"FR_STREAM_LEAVES": "1"}], ids=["unset", "0", "1"])
def test_the_triangle_patch_on_the_simulator(sim, extra):
    """No run-time compiler, no compiled bank: the plan in force leaves the triangle voices to the pull interpreter, and the stream
    answers for that plan what it has always answered -- the same sentence whatever the option says."""
    tree = L.case("tri_128").build()
    answers = []
    for opts in (dict(K.OPTION), dict(K.OPTION, **extra)):
        with Renderer(sim, options=opts) as r:
            synth.install(r, tree)
            r.fill_buffer(2, 0, 16, [np.arange(16, dtype=np.float32)])
            plan = r.plan()
            assert not any(b.get("jit") for b in plan["banks"]), plan["banks"]
            s = plan["stream"]
            with pytest.raises(RenderError) as ei:
                r.stream_begin(2)
            assert ei.value.status == FR_ERR_UNSUPPORTED
            answers.append((s["servable"], s["reason"], s["kernel"], str(ei.value)))
    assert answers[0] == answers[1] and answers[0][0] is False and answers[0][1] != "", answers


@pytest.mark.parametrize("c", [c for c in L.CASES if not c.hostile], ids=[c.name for c in L.CASES if not c.hostile])
def test_expected_rows_meet_the_conditions(sim, c):
    """Input conditions, proven before anything runs on a GPU: over the blocks the GPU test streams, every row of the simulator's
    fr_fill_buffer is at least 95 % finite and louder than 0.01 somewhere (the M-voice cases with M = 4: a voice's row does not
    depend on how many voices there are)."""
    blocks = L.blocks_of(c, [(0, c.frames)])
    assert sum(T for _, T, _ in blocks) == c.frames and max(T for _, T, _ in blocks) == 64 and min(T for _, T, _ in blocks) == 1
    exp = np.concatenate(L.fill_blocks(sim, c.build(L.SIM_M), c.n_rows(L.SIM_M), blocks), axis=1)
    assert exp.shape == (c.n_rows(L.SIM_M), c.frames)
    msg = L.condition_message(c.name, exp)
    assert not msg, msg


def test_expected_rows_of_the_other_sequences(sim):
    """The same conditions for the short blocks, the seeks of tri_am and the store case's edit, which must be audible."""
    for name in ("tri_128", "tri_chunks"):
        c = L.case(name)
        assert not L.condition_message(name, np.concatenate(L.fill_blocks(sim, c.build(), 2, L.short_blocks_of(c)), axis=1))
    c = L.case("tri_am")
    blocks = L.blocks_of(c, SEEKS, seed=31)
    assert not L.condition_message("tri_am seeks", np.concatenate(L.fill_blocks(sim, c.build(), 2, blocks), axis=1))
    c = L.case("tri_env_bus")
    blocks = L.blocks_of(c, [(0, 600)], seed=37)
    tree = c.build()
    a = np.concatenate(L.fill_blocks(sim, tree, 1, blocks, edit_before=9), axis=1)
    b = np.concatenate(L.fill_blocks(sim, tree, 1, blocks), axis=1)
    at = sum(T for _, T, _ in blocks[:9])
    assert not L.condition_message("tri_env_bus edited", a)
    assert K.same_bits(a[:, :at], b[:, :at]) and not K.same_bits(a[:, at:], b[:, at:])


SEEKS = [(0, 300), (9000, 200), (2500, 200)]
