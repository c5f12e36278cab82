"""FR_STREAM_SWEEP on the CPU: the serving rule and the launch rule through the engine's own host code in the host-logic simulator
(tests/sim_tools.py), which has no resident launches -- what the four sweep kernels compute is tests/test_hip_stream_sweep.py's.

Covered here: the option's plumbing and strictness; fr_plan_json["stream"] of every servable case of tests/stream_sweep_cases.py
(servable, kernel, sweep_programs, loop_programs), also under FR_STREAM_STORE; with the option unset or 0 today's sentences word for
word and an unchanged fr_plan_json for three plans without a sweep; with one prerequisite option missing at a time the answer the
engine gives without FR_STREAM_SWEEP; and, before anything runs on a GPU, the conditions on the inputs: every expected row -- the dense
forward reference of the voiceless cases, which the simulator's fr_fill_buffer must equal bit for bit over the same blocks, and the
simulator's fr_fill_buffer of the cases with voices -- is at least 95 % finite and audible."""
import numpy as np
import pytest

import sim_tools
import stream_cases as K
import stream_fx_cases as FX
import stream_loop_cases as SL
import stream_sweep_cases as S
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_CYCLE, FR_ERR_INVALID_ARG, RenderError, Renderer

STREAM_KEYS = ("FR_LOOP_DYN", "FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN",
               "FR_STREAM_HISTORY", "FR_STREAM_EFFECTS", "FR_STREAM_STORE", "FR_STREAM_TAPS", "FR_STREAM_SWEEP", "FR_LOOP_TILES", "FR_STAGE_JIT")


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in STREAM_KEYS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def plan_of(sim, p, options, frames=8):
    """fr_plan_json after one short call of the case under `options`."""
    rows = S.blocks_of(p, [(0, frames)])[0][2]
    with Renderer(sim, options=options) as r:
        p.install(r)
        r.fill_buffer(p.n_rows, 0, len(rows[0]), rows)
        return r.plan()


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_STREAM_SWEEP" not in r.options()
    for v in ("0", "1"):
        with Renderer(sim, options={"FR_STREAM_SWEEP": v}) as r:
            assert r.options()["FR_STREAM_SWEEP"] == {"value": v, "source": "option"}
    clean_env.setenv("FR_STREAM_SWEEP", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_STREAM_SWEEP"] == {"value": "1", "source": "env"}
    with Renderer(sim, options={"FR_STREAM_SWEEP": "0"}) as r:      # the option beats the environment
        assert r.options()["FR_STREAM_SWEEP"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_STREAM_SWEEP", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_STREAM_SWEEP": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_STREAM_SWEEP", bad)
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


@pytest.mark.parametrize("p", S.SERVABLE, ids=S.IDS)
def test_servable_cases(sim, p):
    s = plan_of(sim, p, p.options)["stream"]
    S.check_stream_object(s, p)
    if p.name == "tap_behind":      # rule (b): the tap's program follows the flanger's into its segment; its amount may be 0 frames
        assert s["segments"] == 1 and s["dyn_reads"] == 2 and s["min_ring_delay"] == 0, s
    if p.name == "flanger_64_5":    # the bound is 64: it reads earlier blocks alone
        assert s["min_ring_delay"] == 64 and s["dyn_reads"] == 1, s
    if p.widths and p.name != "tap_behind":
        assert s["min_ring_delay"] == min(p.widths), s


@pytest.mark.parametrize("name", S.STORE_CASES)
def test_store_forms(sim, name):
    p = S.case(name)
    s = plan_of(sim, p, dict(p.options, FR_STREAM_STORE="1"))["stream"]
    S.check_stream_object(s, p, store=True)
    assert s["store"]["on"] is True and s["store"]["inert"] == "", s


@pytest.mark.parametrize("opts", [{}, {"FR_STREAM_SWEEP": "0"}], ids=["unset", "0"])
@pytest.mark.parametrize("p", S.SERVABLE, ids=S.IDS)
def test_unset_or_zero_gives_todays_sentence(sim, p, opts):
    s = plan_of(sim, p, dict(S.without(p.options, "FR_STREAM_SWEEP"), **opts))["stream"]
    assert s["servable"] is False and s["kernel"] == "" and "sweep_programs" not in s, s
    assert s["reason"] == (S.OLD_LOOP_REASON if p.name == "chorus_comb" else S.OLD_SWEEP_REASON), s


NON_SWEEP = [
    ("comb_5_2x128", lambda: K.comb_tree(2, 128, 5), 2, 1, SL.OPTION),
    ("fx_tap_behind", FX.tap_behind_tree, 2, 3, FX.LOOPS),
    ("fx_flanger", FX.flanger_tree, 1, 3, dict(FX.HISTORY, FR_STREAM_DYN="1")),
]


@pytest.mark.parametrize("name,build,n_rows,n_in,options", NON_SWEEP, ids=[c[0] for c in NON_SWEEP])
def test_plans_without_a_sweep_are_unchanged(sim, name, build, n_rows, n_in, options):
    """fr_plan_json with the option unset and 0: the same, key for key; with 1 the stream object gains sweep_programs, all zero, and
    everything else -- the kernel first of all -- stays."""
    tree = build()
    rows = [np.arange(16, dtype=np.float32)] + [np.linspace(0.1, 0.9, 16).astype(np.float32)] * (n_in - 1)
    plans = {}
    for key, extra in (("unset", {}), ("0", {"FR_STREAM_SWEEP": "0"}), ("1", {"FR_STREAM_SWEEP": "1"})):
        with Renderer(sim, options=dict(options, FR_STAGE_JIT="0", **extra)) as r:
            synth.install(r, tree)
            r.fill_buffer(n_rows, 0, 16, rows)
            plans[key] = {k: v for k, v in r.plan().items() if k not in ("build_ms", "lower_ms", "jit_compile_ms")}
    assert plans["unset"]["stream"]["servable"] is True
    assert plans["unset"] == plans["0"]
    on = dict(plans["1"])
    stream = dict(on.pop("stream"))
    assert stream.pop("sweep_programs") == [0] * (sum(stream["programs_per_voice"]) + stream["bus_programs"])
    off = dict(plans["unset"])
    assert stream == off.pop("stream") and on == off


@pytest.mark.parametrize("missing", ["FR_STREAM_PROGRAMS", "FR_STREAM_LOOPS", "FR_STREAM_DYN", "FR_LOOP_DYN"])
@pytest.mark.parametrize("name", ["flanger_8", "voices_base_8", "tap_behind", "chorus_comb"])
def test_one_prerequisite_missing(sim, name, missing):
    """With the option on and one of the options it acts on top of missing, the engine answers what it answers without the option."""
    p = S.case(name)

    def answer(options):
        try:
            plan = plan_of(sim, p, options)
        except RenderError as e:
            return ("error", e.status, str(e))
        return ("plan", plan.get("stream"))
    on = answer(S.without(p.options, missing))
    off = answer(S.without(p.options, missing, "FR_STREAM_SWEEP"))
    if on[0] == "plan" and on[1] is not None:
        on[1].pop("sweep_programs", None)
    if missing == "FR_LOOP_DYN" and name == "chorus_comb":          # (its loop is constant: no sweep plan, FR_LOOP_DYN is no prerequisite)
        assert on[1]["servable"] is True and on[1]["kernel"] == p.kernel()
        return
    assert on == off, (on, off)
    if missing == "FR_LOOP_DYN":
        assert on[0] == "error" and on[1] == FR_ERR_CYCLE, on
    elif missing == "FR_STREAM_PROGRAMS":
        assert on == ("plan", None)
    else:
        assert on[1]["servable"] is False and on[1]["kernel"] == "", on
        if name != "chorus_comb":
            assert on[1]["reason"] == S.OLD_SWEEP_REASON, on
        elif missing == "FR_STREAM_DYN":
            assert on[1]["reason"] == "a program uses S_READ_DYN (a Delay by a signal amount), which block streaming does not serve yet", on


@pytest.mark.parametrize("p", S.SERVABLE, ids=S.IDS)
def test_expected_rows_meet_the_conditions(sim, p):
    """The reference alone, before anything runs on a GPU: over the blocks the GPU test streams, every expected row is at least 95 %
    finite and louder than 0.01 somewhere.  Voiceless: the dense forward reference, which the simulator's fr_fill_buffer of the same
    blocks equals bit for bit; with voices: the simulator's fr_fill_buffer."""
    blocks = S.blocks_of(p, [(0, S.FRAMES)])
    assert sum(T for _, T, _ in blocks) == S.FRAMES and max(T for _, T, _ in blocks) == 64 and min(T for _, T, _ in blocks) == 1
    fill = S.fill_blocks(sim, p, blocks)
    exp = np.concatenate(fill, axis=1)
    if p.voiceless:
        dense = S.dense_reference(p, blocks, "main")
        assert K.same_bits(exp, dense), f"{p.name}: the simulator's fr_fill_buffer against the dense forward reference: " + K.first_diff(exp, dense)
        exp = dense
        lfo = np.concatenate([rows[-1] for _, _, rows in blocks]) if p.n_in == 2 else None
        assert lfo is None or not np.isfinite(lfo).all(), "the LFO / knob row carries the hostile values"
        assert np.isfinite(np.concatenate([rows[0] for _, _, rows in blocks])).all(), "the audio row is finite"
    msg = S.condition_message(p, exp)
    assert not msg, msg


@pytest.mark.parametrize("name", S.SEEK_CASES + ["voices_base_8"])
def test_expected_rows_of_the_other_sequences(sim, name):
    """The same conditions for the short blocks, the seeks and the store cases' edit (on the simulator's fr_fill_buffer)."""
    p = S.case(name)
    for blocks, edit in ((S.short_blocks_of(p), None), (S.blocks_of(p, S.SEEKS, seed=31), None), (S.blocks_of(p, [(0, 600)], seed=37), 9)):
        exp = np.concatenate(S.fill_blocks(sim, p, blocks, edit_before=edit), axis=1)
        msg = S.condition_message(p, exp)
        assert not msg, msg
        if edit is not None:                                         # the edit is audible: what follows differs from the unedited run
            plain = np.concatenate(S.fill_blocks(sim, p, blocks), axis=1)
            at = sum(T for _, T, _ in blocks[:edit])
            assert K.same_bits(exp[:, :at], plain[:, :at]) and not K.same_bits(exp[:, at:], plain[:, at:])


@pytest.mark.parametrize("key,frames,seed,semantics", [("wrap", S.WRAP_FRAMES, 41, "reference"), ("sparkle", S.FRAMES, 43, "sparkle")])
def test_expected_rows_of_the_long_and_the_sparkle_run(key, frames, seed, semantics):
    """The dense forward reference of the flanger of base 8 over the 33 500 frames of the wrap run and, in the Sparkle semantics,
    over its own 1 500 frames: the same conditions."""
    import loop_dyn_reference as ldr
    p = S.case("flanger_8")
    rows = S.concat_rows(S.blocks_of(p, [(0, frames)], seed=seed))
    msg = S.condition_message(p, ldr.render(p.build(), rows, 0, frames, semantics))
    assert not msg, msg
