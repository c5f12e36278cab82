"""FR_STREAM_STORE on the CPU: the option, the serving and launch rule, the zero-frame bring-up and the case table of
tests/stream_store_cases.py, through the engine's own host code in the host-logic simulator and through the C++ oracle.
  * The option is strict, listed once set, and inert without FR_STREAM_PROGRAMS, with FR_DELAY_OBSERVED=1 and with declared track
    slots (fr_plan_json["stream"]["store"]["inert"] says why).
  * fr_plan_json["stream"] names the store form for every patch of the table and has "store"; with the option off the same plan's
    "stream" object is, byte for byte, what a renderer that never heard of the option gives.
  * The first block of a stream that continues brings the rings up to idx as a call of ZERO own frames (csrc/callplan.hpp
    bring_up_form) before the resident launch, which the simulator does not have: the block is refused there, but the bring-up has
    run.  Its launches are the first fr_fill_buffer call's without that call's own frames -- nothing when that call would be
    steady, the look-back window level by level after an edit, a feedback plan's replay, nothing again when FR_RING_KEEP keeps the
    rings -- and the fr_fill_buffer calls that follow, which find the rings current, equal the twin's bit for bit.
  * Two conditions on the table, proven on the oracle so that the GPU tests cannot pass vacuously: every expected row is at least
    95 % finite, and at every boundary of the sequences 1-3 and 5 the oracle rendered WITH A SEEK at the boundary differs from the
    continuing render in at least one sample of the first block after it.
The resident kernel itself is tests/test_hip_stream_store.py; the host rule on its own is tests/test_stream_store_host.py."""
import json

import numpy as np
import pytest

import sim_tools
import stream_reference as SR
import stream_store_cases as S
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, FR_ERR_UNSUPPORTED, FR_OK, RenderError, Renderer

IDS = [S.sequence_id(s) for s in S.SEQUENCES]


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN",
              "FR_STREAM_HISTORY", "FR_STREAM_EFFECTS", "FR_STREAM_STORE", "FR_LOOP_TILES", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def stream_json(r):
    """The text of fr_plan_json's "stream" object, byte for byte (it is the last object before "exchange_stats")."""
    text = r.L.fr_plan_json(r.h).decode()
    at, end = text.find('"stream":'), text.find(',"exchange_stats"')
    assert 0 <= at < end and json.loads("{" + text[at:end] + "}")["stream"] == r.plan()["stream"]
    return text[at:end]


def planned(sim, p, options, raw=False, tracks=None):
    with Renderer(sim, options=options) as r:
        p.install(r)
        if tracks is not None:
            r.set_track_inputs(tracks)
        r.fill_buffer(p.n_rows, 0, 64, S.rows_at(p.name, p.n_in, 0, 64))
        return stream_json(r) if raw else r.plan()


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_STREAM_STORE" not in r.options()
    with Renderer(sim, options={"FR_STREAM_STORE": "1"}) as r:
        assert r.options()["FR_STREAM_STORE"] == {"value": "1", "source": "option"}
    clean_env.setenv("FR_STREAM_STORE", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_STREAM_STORE"] == {"value": "1", "source": "env"}
        assert "FR_STREAM_PROGRAMS" not in r.options()
    with Renderer(sim, options={"FR_STREAM_STORE": "0"}) as r:        # the option beats the environment
        assert r.options()["FR_STREAM_STORE"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_STREAM_STORE", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_STREAM_STORE": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_STREAM_STORE", bad)                      # the environment is read as strictly
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


def test_inert_without_stream_programs(sim):
    p = S.tap_patch()
    assert "stream" not in planned(sim, p, {"FR_STREAM_STORE": "1"})
    said = []
    for options in ({"FR_STREAM_STORE": "1"}, {}):                    # the plain path's refusal, word for word what a renderer without options says
        with Renderer(sim, options=options) as r:
            p.install(r)
            with pytest.raises(RenderError) as ei:
                r.stream_begin(p.n_rows)
            assert ei.value.status == FR_ERR_UNSUPPORTED
            said.append(str(ei.value))
    assert said[0] == said[1]


def test_the_inert_reasons(sim):
    p = S.tap_patch()
    off = planned(sim, p, dict(p.options, FR_DELAY_OBSERVED="1"))["stream"]
    s = planned(sim, p, dict(p.options, **S.STORE, FR_DELAY_OBSERVED="1"))["stream"]
    assert s["store"] == {"on": False, "slots": [], "continued": False, "relaunches": 0,
                          "inert": "FR_DELAY_OBSERVED=1: streamed rows would escape the observed bounds"}, s
    assert {k: v for k, v in s.items() if k != "store"} == off
    s = planned(sim, p, dict(p.options, **S.STORE), tracks=8)["stream"]
    assert s["store"]["on"] is False and s["store"]["inert"] == "declared track slots" and s["kernel"] not in (S.NEW_KERNEL, S.NEW_FX_KERNEL), s


@pytest.mark.parametrize("name", list(S.PATCHES))
def test_the_plan_names_the_store_form(sim, name):
    p = S.PATCHES[name]()
    off_plain = planned(sim, p, p.options, raw=True)
    assert planned(sim, p, dict(p.options, FR_STREAM_STORE="0"), raw=True) == off_plain and '"store"' not in off_plain
    assert S.NEW_KERNEL not in off_plain and S.NEW_FX_KERNEL not in off_plain
    off, on = planned(sim, p, p.options)["stream"], planned(sim, p, dict(p.options, **S.STORE))["stream"]
    assert on["servable"] is True and on["kernel"] == (S.NEW_FX_KERNEL if p.voiceless else S.NEW_KERNEL), on
    assert on["store"] == {"on": True, "slots": list(range(p.n_in)), "continued": False, "relaunches": 0, "inert": ""}, on
    assert list(on)[-2:] == ["store", "kernel"]
    assert {k: v for k, v in on.items() if k not in ("store", "kernel")} == {k: v for k, v in off.items() if k != "kernel"}


def test_one_balanced_bank_that_writes_rows_takes_the_program_path(sim):
    from libfriendship_amd import synth
    tree = synth.additive_tree(n_voices=2, n_partials=128, seed=3)
    for options, kernel in ((S.PROGRAMS, ""), (S.STORE, S.NEW_KERNEL)):
        with Renderer(sim, options=options) as r:
            synth.install(r, tree)
            r.fill_buffer(2, 0, 64, [synth.time_ramp(0, 64)])
            s = r.plan()["stream"]
            assert s["kernel"] == kernel and s["servable"] is True and s["programs_per_voice"] == [0, 0], s


def test_more_slots_than_the_kernel_streams(sim):
    """Nine fed slots: fr_stream_begin is refused with the count and the limit, and the renderer goes on with fr_fill_buffer
    without a seek (the twin's samples)."""
    p = S.tap_patch()
    rows = lambda idx, T: S.rows_at(p.name, 9, idx, T)
    with Renderer(sim, options=dict(p.options, **S.STORE)) as r, Renderer(sim) as f:
        p.install(r)
        p.install(f)
        a = r.fill_buffer(p.n_rows, 0, 150, rows(0, 150))
        with pytest.raises(RenderError) as ei:
            r.stream_begin(p.n_rows)
        assert ei.value.status == FR_ERR_UNSUPPORTED and "9 slots" in str(ei.value) and "at most 8" in str(ei.value), str(ei.value)
        assert not SR.first_diff(a, f.fill_buffer(p.n_rows, 0, 150, rows(0, 150)), "before")
        assert not SR.first_diff(r.fill_buffer(p.n_rows, 150, 214, rows(150, 64)), f.fill_buffer(p.n_rows, 150, 214, rows(150, 64)), "after the refusal")


def test_a_block_with_more_slots_than_the_kernel_streams(sim):
    """The same at a block: fr_stream_begin passes (nothing is fed yet), the first block with nine rows is refused with the count
    and the limit before anything is touched, and fr_fill_buffer goes on from the renderer's head with the twin's samples."""
    p = S.late_slots_patch()
    with Renderer(sim, options=dict(p.options, **S.STORE)) as r, Renderer(sim) as f:
        p.install(r)
        p.install(f)
        r.stream_begin(p.n_rows)
        with pytest.raises(RenderError) as ei:
            r.stream_block_rows(0, S.rows_at(p.name, 9, 0, 64), n_times=64)
        assert ei.value.status == FR_ERR_UNSUPPORTED and "9 slots" in str(ei.value) and "at most 8" in str(ei.value), str(ei.value)
        for idx, T in ((0, 64), (64, 150)):
            rows = S.rows_at(p.name, 3, idx, T)
            assert not SR.first_diff(r.fill_buffer(p.n_rows, idx, idx + T, rows), f.fill_buffer(p.n_rows, idx, idx + T, rows), "after the refused block")


def _rows_before(p, steps, upto):
    n = p.n_rows
    for s in steps[:upto]:
        if s[0] == "edit":
            n = getattr(p, "rows_after", {}).get(s[1], n)
    return n


def _expected_bring_up(first_call, T):
    """What the zero-frame bring-up must launch, from the twin's first call at the boundary (its fr_plan_json launches): that
    call's launches over the frames before idx -- every stage launch of form levels or replay and every bank launch of a window
    longer than the call, each shortened by the call's own T frames; none when the call is steady."""
    stage = sorted((x["form"], x["frames"] - (T if x["form"] == "levels" else 0)) for x in first_call["stage_launches"]
                   if x["form"] in ("replay", "repair") or (x["form"] == "levels" and x["frames"] > T))   # (a steady call may run level by level too)
    replay = any(form == "replay" for form, _ in stage)                 # (a replay's windows end at idx; a look-back window ends with the call)
    banks = sorted(x["frames"] - (T if x.get("form", "call") == "call" and not replay else 0) for x in first_call["bank_launches"]
                   if x["frames"] > T or x.get("form", "call") != "call")
    return stage, banks


@pytest.mark.parametrize("keep", [False, True], ids=["", "ring_keep"])
@pytest.mark.parametrize("seq", [s for s in S.SEQUENCES if s[0] in ("fill_then_stream", "stream_edit_stream", "row_rules")],
                         ids=[S.sequence_id(s) for s in S.SEQUENCES if s[0] in ("fill_then_stream", "stream_edit_stream", "row_rules")])
def test_the_zero_frame_bring_up_is_the_first_call_s(sim, seq, keep):
    extra = {"FR_RING_KEEP": "1"} if keep else {}
    p, steps, bounds, options = S.build(seq)
    (b,) = bounds
    _, idx, T, rows = steps[b]
    with Renderer(sim, options=extra) as f:                             # the twin, and its first call at the boundary
        p2 = S.build(seq)[0]
        p2.install(f)
        twin = S.run(f, p2, steps[:b], streamed=False)
        twin += S.run(f, p2, steps[b:b + 1], streamed=False, n_rows=_rows_before(p2, steps, b))
        first_call = f.plan()
        twin += S.run(f, p2, steps[b + 1:], streamed=False, n_rows=_rows_before(p2, steps, b))
    with Renderer(sim, options=dict(options, **S.STORE, **extra)) as r:
        p.install(r)
        got = S.run(r, p, steps[:b], streamed=False)
        n_rows = _rows_before(p, steps, b)
        r.stream_begin(n_rows)
        with pytest.raises(RenderError):                                # (the simulator has no resident launch; the bring-up ran before it)
            r.stream_block_rows(idx, rows, n_times=T)
        plan = r.plan()
        stage = sorted((x["form"], x["frames"]) for x in plan["stage_launches"])
        banks = sorted(x["frames"] for x in plan["bank_launches"])
        assert (stage, banks) == _expected_bring_up(first_call, T), (stage, banks, first_call["stage_launches"], first_call["bank_launches"])
        got += S.run(r, p, steps[b:], streamed=False, n_rows=n_rows)    # closes the stream; the rings are current at idx
    assert len(got) == len(twin)
    for k, ((st, a), (st_t, t)) in enumerate(zip(got, twin)):
        assert st == st_t and (st != FR_OK or not SR.first_diff(a, t, f"{S.sequence_id(seq)}: result {k}"))


# ---- the table itself, on the oracle ---------------------------------------------------------------------------------------------

_ORACLE = {}


def oracle_of(oracle_lib, seq, seek_at=()):
    key = (S.sequence_id(seq), tuple(seek_at))
    if key not in _ORACLE:
        p, steps, bounds, _ = S.build(seq)
        upto = next((k for k, s in enumerate(steps) if s[0] in ("fill", "block") and s[1] > 2000), None)
        with Renderer(oracle_lib) as o:
            p.install(o)
            _ORACLE[key] = (steps[:upto], bounds, S.run(o, p, steps[:upto], streamed=False, seek_at=seek_at))
    return _ORACLE[key]


@pytest.mark.parametrize("seq", S.SEQUENCES, ids=IDS)
def test_every_expected_row_is_mostly_finite(oracle_lib, seq):
    steps, _, out = oracle_of(oracle_lib, seq)
    blocks = [a for st, a in out if st == FR_OK]
    rows = max(a.shape[0] for a in blocks)
    share = SR.finite_share([a for a in blocks if a.shape[0] == rows])
    assert (share >= S.FINITE_SHARE).all(), share
    whole = np.concatenate([a for a in blocks if a.shape[0] == rows], axis=1)
    assert (np.abs(np.where(np.isfinite(whole), whole, 0)).max(axis=1) > 0).all()            # no row is silent


@pytest.mark.parametrize("seq", [s for s in S.SEQUENCES if s[0] != "seeks"], ids=[i for i, s in zip(IDS, S.SEQUENCES) if s[0] != "seeks"])
def test_a_seek_at_a_boundary_shows_in_the_first_block_after_it(oracle_lib, seq):
    steps, bounds, cont = oracle_of(oracle_lib, seq)
    assert bounds
    at = S.rendered_steps(steps)
    for b in bounds:
        _, _, seek = oracle_of(oracle_lib, seq, seek_at=(b,))
        k = at.index(b)
        assert cont[k][0] == seek[k][0] == FR_OK
        differ = (cont[k][1].view(np.uint32) != seek[k][1].view(np.uint32)).sum()
        print(f"{S.sequence_id(seq)}: {differ} of {cont[k][1].size} samples of the first block after step {b} differ with a seek there")
        assert differ >= 1, "a seek at this boundary cannot be told from continuing: a broken case"
        for j in range(k):
            assert cont[j][0] == seek[j][0] and (cont[j][0] != FR_OK or not SR.first_diff(seek[j][1], cont[j][1], "before the boundary"))
