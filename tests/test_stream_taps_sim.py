"""FR_STREAM_TAPS on the CPU: the serving rule of block streaming for short and signal delays of computed values
(csrc/streamplan.hpp) through the engine's own host code in the host-logic simulator, and the proof of what
tests/test_hip_stream_taps.py then relies on.
  * With FR_STREAM_PROGRAMS and FR_STREAM_TAPS on, every case of tests/stream_taps_cases.py is served in its level form:
    fr_plan_json's "stream" names the kernel where the plan alone decides it (the prog and the bus kernel are named by a launch,
    which the simulator does not make: there the name is "", and the launch rule's choice is pinned by
    tests/cpp/streamtaps_tests.cpp on hand-built plans and by the device test), counts the levels, the reads below a block of rings that
    programs store and the signal reads among them, the programs of each voice, the bus programs and the segments.
  * Without FR_STREAM_TAPS every case is refused with today's sentence; with the option absent or "0" the text of the "stream"
    object is, byte for byte, that of a renderer that never heard of it -- for these patches and for one patch each of the loops,
    dyn, fx and store case files.  What stays refused says so, word for word.
  * Two more patches put FR_STREAM_TAPS next to FR_STREAM_HISTORY and next to FR_STREAM_BANKS (stream_taps_cases.COMPOSED): the
    hist and the banks kernel take a level form as it is.  They go through every test here and on the device like the eight.
  * The dense reference (tests/stream_reference.py) equals the simulator's fr_fill_buffer of every block of every case, and the
    C++ oracle over the first 300 frames.
  * Conditions on the chosen inputs: every output row of the reference is at least 95 % finite; raising every constant Delay by one
    frame changes at least 90 % of the finite samples of every row behind one, over both whole streams; raising a signal amount by
    one frame -- the base of a chorus, the knob's row of fx_product_knob_delay -- changes at least half of the finite samples of every
    row, over each whole stream.
The simulator has no resident launches: the kernels are tests/test_hip_stream_taps.py; the rule on hand-built plans, the launch
rule and a host model of a voice's chain of programs are tests/test_stream_taps_host.py."""
import json

import numpy as np
import pytest

import sim_tools
import stream_dyn_cases as D
import stream_fx_cases as F
import stream_loop_cases as L
import stream_reference as SR
import stream_store_cases as S
import stream_taps_cases as T
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, FR_ERR_UNSUPPORTED, RenderError, Renderer

NAMES = [c["name"] for c in T.ALL]


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture(scope="module")
def trees():
    """Every case's graph, built once."""
    t = {c["name"]: c["build"]() for c in T.ALL}
    t.update({c[0]: c[1]() for c in T.REFUSED})
    return t


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN",
              "FR_STREAM_HISTORY", "FR_STREAM_EFFECTS", "FR_STREAM_STORE", "FR_STREAM_TAPS", "FR_LOOP_TILES", "FR_RING_KEEP", "FR_TRACK_HISTORY",
              "FR_DELAY_OBSERVED", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def stream_json(r):
    """The text of fr_plan_json's "stream" object, byte for byte (it is the last object before "exchange_stats")."""
    text = r.L.fr_plan_json(r.h).decode()
    at, end = text.find('"stream":'), text.find(',"exchange_stats"')
    assert 0 <= at < end and json.loads("{" + text[at:end] + "}")["stream"] == r.plan()["stream"]
    return text[at:end]


def plan_of(sim, tree, n_rows, options, n_in=1, semantics="reference", raw=False):
    with Renderer(sim, semantics=semantics, options=options) as r:
        synth.install(r, tree)
        r.fill_buffer(n_rows, 0, 64, [synth.time_ramp(0, 64)] + [np.ones(64, np.float32)] * (n_in - 1))
        assert ("FR_STREAM_TAPS" in r.options()) == ("FR_STREAM_TAPS" in options)
        return stream_json(r) if raw else r.plan()


@pytest.mark.parametrize("name", NAMES)
def test_servable_with_the_option(sim, trees, name):
    c = T.case(name)
    plan = plan_of(sim, trees[name], c["n_rows"], c["options"], c["n_in"])
    assert plan["fused_programs"] == 0                # no fused form: what is served is the level form
    s = plan["stream"]
    T.check_stream_object(s, c)
    with Renderer(sim, options=c["options"]) as r:   # fr_stream_begin builds the tables (the simulator launches nothing)
        synth.install(r, trees[name])
        r.stream_begin(c["n_rows"])
        with pytest.raises(RenderError):
            r.stream_block_rows(0, [synth.time_ramp(0, 8)] * len(s["input_slots"]))
        r.fill_buffer(c["n_rows"], 0, 16, [synth.time_ramp(0, 16)] * c["n_in"])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("others", ["its_own", "all_nine"])
def test_refused_without_the_option(sim, trees, name, others):
    """Today's sentence, with the case's other options and with every serving option there was before this one."""
    c = T.case(name)
    options = T.without(c["options"], "FR_STREAM_TAPS") if others == "its_own" else T.ALL_BEFORE
    assert len(T.ALL_BEFORE) == 9 and "FR_STREAM_TAPS" not in T.ALL_BEFORE
    s = plan_of(sim, trees[name], c["n_rows"], options, c["n_in"])["stream"]
    assert s["servable"] is False and s["reason"] == T.NO_FUSED_FORM, s
    assert not any(k in s for k in T.NEW_KEYS), s
    with Renderer(sim, options=options) as r:
        synth.install(r, trees[name])
        with pytest.raises(RenderError) as ei:
            r.stream_begin(c["n_rows"])
        assert ei.value.status == FR_ERR_UNSUPPORTED and T.NO_FUSED_FORM in str(ei.value)
        r.fill_buffer(c["n_rows"], 64, 80, [synth.time_ramp(64, 80)] + [np.ones(16, np.float32)] * (c["n_in"] - 1))


@pytest.mark.parametrize("name", [c[0] for c in T.REFUSED])
def test_what_stays_refused(sim, trees, name):
    _, _, n_rows, options, n_in, why = next(r for r in T.REFUSED if r[0] == name)
    assert options.get("FR_STREAM_TAPS") == "1"
    s = plan_of(sim, trees[name], n_rows, options, n_in)["stream"]
    assert s["servable"] is False and s["reason"] == why, s
    with Renderer(sim, options=options) as r:
        synth.install(r, trees[name])
        with pytest.raises(RenderError) as ei:
            r.stream_begin(n_rows)
        assert ei.value.status == FR_ERR_UNSUPPORTED and why in str(ei.value)
        r.fill_buffer(n_rows, 64, 80, [synth.time_ramp(64, 80)] + [np.ones(16, np.float32)] * (n_in - 1))


def test_a_signal_delay_inside_a_loop_program_stays_refused(sim):
    """_DYN ops inside loop programs: the rule's own sentence, with or without the option (the patch delays the VOICE by a signal
    amount inside a comb of 5 frames; its plan is built and fr_fill_buffer renders it)."""
    tree = L.dyn_loop_tree(2, 128)
    said = []
    for options in (dict(T.ALL_BEFORE, FR_STREAM_TAPS="1"), T.ALL_BEFORE):
        s = plan_of(sim, tree, 2, options)["stream"]
        assert s["servable"] is False
        said.append(s["reason"])
    assert said[0] == said[1] and "a loop program uses S_READ_DYN" in said[0]


def test_a_feedback_plan_with_a_signal_delay_of_a_computed_value_is_the_planner_s_refusal(sim):
    """x = voice + 0.6 * Delay(x, 5); y = x + Delay(x, 1 + 30 * lfo): out of the rule's reach -- the planner itself refuses the plan
    (fr_status 10), for fr_fill_buffer too, with or without the option."""
    g = synth.GraphArrays()
    x = L._loop(g, D._voices(g, 2, 128), [(5, 0.6)], 2)
    tree = D._to_rows(g, g.binop(synth.K_SUM2, x, D._delay(g, x, D._lfo_amount(g), 2), 2))
    said = []
    for options in ({}, T.ALL_BEFORE, dict(T.ALL_BEFORE, FR_STREAM_TAPS="1")):
        with Renderer(sim, options=options) as r:
            synth.install(r, tree)
            with pytest.raises(RenderError) as ei:
                r.fill_buffer(2, 0, 64, [synth.time_ramp(0, 64)])
            assert ei.value.status == FR_ERR_UNSUPPORTED == 10
            said.append(str(ei.value))
    assert said[0] == said[1] == said[2] and "a feedback plan reads a program's ring through a signal-dependent Delay" in said[0]


def _others():
    """One patch each of the loops, dyn, fx and store case files, with the options that serve it."""
    store = S.PATCHES["tap_100"]()
    return [("comb_5_2x128", L.case("comb_5_2x128")["build"](), 2, L.OPTION, 1),
            ("chorus_short", D.case("chorus_short")["build"](), 2, D.OPTION, 1),
            ("tap_behind", F.case("tap_behind")["build"](), 2, F.case("tap_behind")["options"], 3),
            ("tap_100", store.tree, store.n_rows, dict(store.options, FR_STREAM_STORE="1"), store.n_in)]


@pytest.mark.parametrize("off", [None, "0"])
def test_without_the_option_every_answer_is_today_s(sim, trees, off):
    """The option absent, and "0": the text of fr_plan_json's "stream" object is, byte for byte, what a renderer that never heard
    of the option gives."""
    patches = _others() + [(c["name"], trees[c["name"]], c["n_rows"], c["options"], c["n_in"]) for c in T.SERVABLE]
    for name, tree, n_rows, options, n_in in patches:
        plain = plan_of(sim, tree, n_rows, T.without(options, "FR_STREAM_TAPS"), n_in, raw=True)
        got = plan_of(sim, tree, n_rows, T.without(options, "FR_STREAM_TAPS") if off is None else dict(options, FR_STREAM_TAPS=off), n_in, raw=True)
        assert got == plain and '"stream":{' in got, name
        assert not any(f'"{k}"' in got for k in T.NEW_KEYS), name
        if name in NAMES:
            assert T.NO_FUSED_FORM in got and '"servable":false' in got, name
        else:
            assert '"servable":true' in got, name


def test_a_plan_that_was_served_keeps_its_stream_object(sim):
    """With the option on, a plan with a fused form, a one-level plan and a feedback plan have the object they had plus the three
    keys: one level, and the short reads they always had (the tap behind a loop, a loop's own reads)."""
    for name, tree, n_rows, options, n_in in _others():
        a = plan_of(sim, tree, n_rows, options, n_in)["stream"]
        b = plan_of(sim, tree, n_rows, dict(options, FR_STREAM_TAPS="1"), n_in)["stream"]
        assert a["servable"] is True and not any(k in a for k in T.NEW_KEYS), a
        stripped = {k: v for k, v in b.items() if k not in T.NEW_KEYS}
        assert stripped == a and list(stripped) == list(a), name
        assert b["levels"] == 1 and b["dyn_ring_reads"] == 0, b


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_STREAM_TAPS" not in r.options()
    with Renderer(sim, options=T.OPTION) as r:
        assert r.options()["FR_STREAM_TAPS"] == {"value": "1", "source": "option"}
    clean_env.setenv("FR_STREAM_TAPS", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_STREAM_TAPS"] == {"value": "1", "source": "env"}
        assert "FR_STREAM_PROGRAMS" not in r.options()
    with Renderer(sim, options={"FR_STREAM_TAPS": "0"}) as r:         # the option beats the environment
        assert r.options()["FR_STREAM_TAPS"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_STREAM_TAPS", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_STREAM_TAPS": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_STREAM_TAPS", bad)                       # the environment is read as strictly
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


def test_inert_without_stream_programs(sim, trees):
    tree = trees["env_fir_2x128"]
    assert "stream" not in plan_of(sim, tree, 2, {"FR_STREAM_TAPS": "1"})
    said = []
    for options in ({"FR_STREAM_TAPS": "1"}, {}):                     # the plain path's refusal, word for word what a renderer without options says
        with Renderer(sim, options=options) as r:
            synth.install(r, tree)
            with pytest.raises(RenderError) as ei:
                r.stream_begin(2)
            assert ei.value.status == FR_ERR_UNSUPPORTED
            said.append(str(ei.value))
    assert said[0] == said[1]


# ---- the dense reference and the inputs, before any GPU run -----------------------------------------------------------------------

def test_the_sequence_is_the_one_described():
    import stream_cases as K
    for c in T.ALL:
        streams = T.streams_of(c)
        assert [len(b) for b in streams] == [12, 4] and T.frames_of(c) == 572 and c["oracle_frames"] == 300
        assert [n for _, n, _ in streams[0][:8]] == list(K.FIRST_LENGTHS) + [5]
        assert [[idx for idx, _, _ in b] for b in streams][1][0] == 0 and streams[0][8][0] == 5003 and streams[0][10][0] == 69
        assert all(len(rows) == c["n_in"] and all(len(r) == n for r in rows) for b in streams for _, n, rows in b)


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_equals_the_simulator(sim, name):
    c = T.case(name)
    tree, streams, expected = T.reference_of(name)
    n = 0
    for s, (blocks, exp) in enumerate(zip(streams, expected)):
        with Renderer(sim) as f:
            synth.install(f, tree)
            for k, ((idx, n_t, rows), e) in enumerate(zip(blocks, exp)):
                got = f.fill_buffer(c["n_rows"], idx, idx + n_t, rows)
                assert not SR.first_diff(got, e, f"{name} stream {s} block {k} at frame {idx} (T={n_t}), fr_fill_buffer against the reference")
                n += n_t
    assert n == T.frames_of(c)


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_equals_the_oracle(oracle_lib, name):
    c = T.case(name)
    tree, streams, expected = T.reference_of(name)
    n = 0
    with Renderer(oracle_lib) as o:
        synth.install(o, tree)
        for k, ((idx, n_t, rows), e) in enumerate(zip(streams[0], expected[0])):
            n_t = min(n_t, c["oracle_frames"] - idx)
            if n_t <= 0:
                break
            got = o.fill_buffer(c["n_rows"], idx, idx + n_t, [r[:n_t] for r in rows])
            assert not SR.first_diff(got, e[:, :n_t], f"{name} block {k} at frame {idx} (T={n_t}), the oracle against the reference")
            n += n_t
    assert n == c["oracle_frames"] == 300


@pytest.mark.parametrize("name", NAMES)
def test_every_row_is_mostly_finite(name):
    _, _, expected = T.reference_of(name)
    share = SR.finite_share([a for exp in expected for a in exp])
    print(f"{name}: finite share per row, lowest {share.min():.4f}")
    assert (share >= T.FINITE_SHARE).all(), share
    whole = np.concatenate([a for exp in expected for a in exp], axis=1)
    assert (np.abs(np.where(np.isfinite(whole), whole, 0)).max(axis=1) > 0).all()        # no row of the reference is silent
    assert max(float(np.abs(np.where(np.isfinite(a), a, 0)).max()) for exp in expected for a in exp) > 0.01


def _changed_share(name, other_tree, rows):
    """Per row of `rows`, per stream: the share of the reference's finite samples that `other_tree` renders differently."""
    c = T.case(name)
    _, streams, expected = T.reference_of(name)
    out = []
    for s, (blocks, exp) in enumerate(zip(streams, expected)):
        ref = np.concatenate(exp, axis=1)
        off = np.concatenate(SR.expected_blocks(other_tree, blocks, c["semantics"]), axis=1)
        for r in rows:
            finite = np.isfinite(ref[r])
            out.append((s, r, float((ref[r].view(np.uint32) != off[r].view(np.uint32))[finite].mean()), int(finite.sum())))
    return out


def _changed_share(name, other_tree, rows, other_streams=None):
    """Per stream and per row of `rows`: the share of the reference's finite samples that `other_tree`, fed `other_streams`
    (default: the case's own), renders differently -- over the whole stream, the frames behind each seek included."""
    c = T.case(name)
    _, streams, expected = T.reference_of(name)
    out = []
    for s, (blocks, exp) in enumerate(zip(streams, expected)):
        ref = np.concatenate(exp, axis=1)
        off = np.concatenate(SR.expected_blocks(other_tree, blocks if other_streams is None else other_streams[s], c["semantics"]), axis=1)
        for r in rows:
            finite = np.isfinite(ref[r])
            out.append((s, r, float((ref[r].view(np.uint32) != off[r].view(np.uint32))[finite].mean()), int(finite.sum())))
    return out


@pytest.mark.parametrize("name", [c["name"] for c in T.ALL if c["delay_rows"]])
def test_a_delay_one_frame_off_shows(name):
    """Every constant Delay one frame longer, over all the finite samples of every row behind one, in each whole stream: the first
    frames of a stream and of each segment behind a seek, where both delays still read the zeros of the past, are counted too."""
    c = T.case(name)
    tree, _, _ = T.reference_of(name)
    assert SR.rows_behind_constant_delays(tree) == c["delay_rows"]
    for s, r, differ, n in _changed_share(name, SR.with_delays_raised(tree), c["delay_rows"]):
        print(f"{name} stream {s} row {r}: {differ:.4f} of {n} finite samples differ with every constant delay one frame longer")
        assert differ >= T.SENSITIVITY, (s, r, differ)


@pytest.mark.parametrize("name", [c["name"] for c in T.ALL if c["signal"] or c["knob"]])
def test_a_signal_amount_one_frame_off_shows(name):
    """The signal amount raised by one frame, over each whole stream (the one with the seek to 5003, whose past is zeros, included):
    the base of a chorus' amount in the graph; of fx_product_knob_delay the amount's row itself (slot 3), every frame of it."""
    c = T.case(name)
    assert len([x for x in T.ALL if x["dyn_ring"]]) == len([x for x in T.ALL if x["signal"] or x["knob"]])   # every case with a signal delay is here
    if c["knob"]:
        tree, _, _ = T.reference_of(name)
        shares = _changed_share(name, tree, range(c["n_rows"]), T.streams_of(c, knob_raised=1.0))
    else:
        shares = _changed_share(name, c["signal"](), range(c["n_rows"]))
    for s, r, differ, n in shares:
        print(f"{name} stream {s} row {r}: {differ:.4f} of {n} finite samples differ with the amount one frame higher")
        assert differ >= T.SIGNAL_SENSITIVITY, (s, r, differ)


def test_the_knob_s_amounts_are_the_ones_described():
    """fx_product_knob_delay's amount row: mostly inside (0, 48), and it hits 0 frames, the bound and beyond it in every stream."""
    for blocks in T.streams_of(T.case("fx_product_knob_delay")):
        a = np.concatenate([rows[3] for _, _, rows in blocks])
        assert np.isfinite(a).all() and (a >= 0).all() and ((a > 0) & (a < 48)).mean() > 0.6
        assert (a == 0).any() and (a >= 48).any() and (a != np.floor(a)).any()                          # 0 frames, the bound, fractional amounts


def test_the_edit_sequence(sim):
    """The GPU test's edit between two streams: the second patch's reference from frame 0 equals fr_fill_buffer of a renderer that
    had the first patch installed and rendered before."""
    a, b = T.case("env_fir_2x128"), T.case("bus_chorus_3x128")
    _, streams_b, exp_b = T.reference_of(b["name"])
    _, streams_a, _ = T.reference_of(a["name"])
    with Renderer(sim) as f:
        synth.install(f, a["build"]())
        for idx, n_t, rows in streams_a[1]:
            f.fill_buffer(a["n_rows"], idx, idx + n_t, rows)
        synth.install(f, b["build"]())
        for k, ((idx, n_t, rows), e) in enumerate(zip(streams_b[1], exp_b[1])):
            assert not SR.first_diff(f.fill_buffer(b["n_rows"], idx, idx + n_t, rows), e, f"block {k} at frame {idx} after the edit")


def test_the_depth_edit_is_the_edited_tree(sim):
    """The GPU test's edit inside a stream that stores its rows: fr_fill_buffer of env_chorus, the depth edited through the edge
    calls, fr_fill_buffer on -- equals the dense reference of the edited tree where the edit has taken effect, and differs from the
    unedited one (the edit shows)."""
    c = T.case("env_chorus_2x128")
    tree, streams, _ = T.reference_of(c["name"])
    blocks = streams[0][:8]                                              # the first segment: 300 frames from 0
    cut = 4
    before = SR.expected_blocks(tree, blocks)
    after = SR.expected_blocks(T.with_depth(tree), blocks)
    with Renderer(sim) as f:
        synth.install(f, tree)
        got = [f.fill_buffer(2, idx, idx + n_t, rows) for idx, n_t, rows in blocks[:cut]]
        T.edit_depth(f, tree)
        got += [f.fill_buffer(2, idx, idx + n_t, rows) for idx, n_t, rows in blocks[cut:]]
    for k, (g, b, a) in enumerate(zip(got, before, after)):
        assert not SR.first_diff(g, b if k < cut else a, f"block {k}")
    assert any((a.view(np.uint32) != b.view(np.uint32)).mean() > 0.5 for a, b in zip(after[cut:], before[cut:]))
