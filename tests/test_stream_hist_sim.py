"""FR_STREAM_HISTORY on the CPU: the serving rule of block streaming for delayed reads of input rows (csrc/streamplan.hpp) through
the engine's own host code in the host-logic simulator, and the proof of what tests/test_hip_stream_hist.py then relies on.
  * With FR_STREAM_PROGRAMS and FR_STREAM_HISTORY on, every case of tests/stream_hist_cases.py is served: fr_plan_json's "stream"
    counts the reads ("hist_reads", "hist_dyn_reads"), gives the deepest of them ("input_lookback") and names the kernel; what
    stays refused says so; with the option absent or 0 every answer is what it is without the key.
  * The dense reference (tests/stream_reference.py) equals the simulator's fr_fill_buffer of every block of every case, and the
    C++ oracle as far as its budget reaches: it handles a Delay of an input before the GPU test compares with it.
  * Conditions on the chosen inputs: every output row of the reference is at least 95 % finite, and raising every constant
    Delay by one frame changes at least 90 % of the finite samples of every row it feeds -- control rows are uniform random
    numbers and the time row is a ramp, so a sample read one frame late is another number almost everywhere; the hostile
    constants (-2.5 next to -2.5) and the frames before the delay has elapsed are the rest.
The simulator has no resident launches: the kernel itself is tests/test_hip_stream_hist.py; the rule on hand-built plans, the
launch check and a host model of the history are tests/test_stream_hist_host.py."""
import numpy as np
import pytest

import sim_tools
import stream_cases as K
import stream_hist_cases as H
import stream_reference as SR
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, FR_ERR_UNSUPPORTED, RenderError, Renderer

NAMES = [c["name"] for c in H.SERVABLE]


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture(scope="module")
def trees():
    """Every case's graph, built once."""
    t = {c["name"]: c["build"]() for c in H.SERVABLE}
    t.update({c[0]: c[1]() for c in H.REFUSED})
    return t


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN",
              "FR_STREAM_HISTORY", "FR_LOOP_TILES", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def plan_of(sim, tree, n_rows, options, n_in=1, semantics="reference"):
    with Renderer(sim, semantics=semantics, options=options) as r:
        synth.install(r, tree)
        r.fill_buffer(n_rows, 0, 64, [synth.time_ramp(0, 64)] + [np.ones(64, np.float32)] * (n_in - 1))
        assert ("FR_STREAM_HISTORY" in r.options()) == ("FR_STREAM_HISTORY" in options)
        return r.plan()


def without(options):
    return {k: v for k, v in options.items() if k != "FR_STREAM_HISTORY"}


@pytest.mark.parametrize("name", NAMES)
def test_servable_with_the_option(sim, trees, name):
    c = H.case(name)
    s = plan_of(sim, trees[name], c["n_rows"], c["options"], c["n_in"], c["semantics"])["stream"]
    H.check_stream_object(s, c)
    with Renderer(sim, semantics=c["semantics"], options=c["options"]) as r:   # fr_stream_begin builds the tables (the simulator launches nothing)
        synth.install(r, trees[name])
        r.stream_begin(c["n_rows"])
        with pytest.raises(RenderError):
            r.stream_block_rows(0, [synth.time_ramp(0, 8)] * len(s["input_slots"]))
        r.fill_buffer(c["n_rows"], 0, 16, [synth.time_ramp(0, 16)] * c["n_in"])


@pytest.mark.parametrize("name", [c[0] for c in H.REFUSED])
def test_refused(sim, trees, name):
    _, _, n_rows, options, n_in, why = K.case(H.REFUSED, name)
    s = plan_of(sim, trees[name], n_rows, options, n_in)["stream"]
    assert s["servable"] is False and all(w in s["reason"] for w in why), s
    assert s["kernel"] != H.NEW_KERNEL and all(k in s for k in H.NEW_KEYS) == ("FR_STREAM_HISTORY" in options)
    with Renderer(sim, options=options) as r:
        synth.install(r, trees[name])
        with pytest.raises(RenderError) as ei:
            r.stream_begin(n_rows)
        assert ei.value.status == FR_ERR_UNSUPPORTED and all(w in str(ei.value) for w in why)
        r.fill_buffer(n_rows, 64, 80, [synth.time_ramp(64, 80)] + [np.ones(16, np.float32)] * (n_in - 1))


@pytest.mark.parametrize("name", NAMES + [c[0] for c in H.REFUSED])
@pytest.mark.parametrize("off", [None, "0"])
def test_without_the_option_every_answer_is_today_s(sim, trees, name, off):
    """The option absent, and "0": fr_plan_json["stream"] is, key for key and in the same order, what a renderer without the key
    gives -- a refusal with one of the two old texts for every servable case."""
    if name in NAMES:
        c = H.case(name)
        n_rows, options, n_in = c["n_rows"], c["options"], c["n_in"]
    else:
        _, _, n_rows, options, n_in, _ = K.case(H.REFUSED, name)
    plain = plan_of(sim, trees[name], n_rows, without(options), n_in)["stream"]
    s = plan_of(sim, trees[name], n_rows, without(options) if off is None else dict(options, FR_STREAM_HISTORY=off), n_in)["stream"]
    assert s == plain and list(s) == list(plain)
    assert not any(k in s for k in H.NEW_KEYS) and s["kernel"] != H.NEW_KERNEL
    if name in NAMES:
        assert s["servable"] is False and s["reason"] in (H.OLD_INPUT, H.OLD_INPUT_DYN), s
        with Renderer(sim, options=without(options)) as r:
            synth.install(r, trees[name])
            with pytest.raises(RenderError) as ei:
                r.stream_begin(n_rows)
            assert ei.value.status == FR_ERR_UNSUPPORTED and s["reason"] in str(ei.value)


def test_a_plan_without_a_delayed_input_keeps_its_stream_object(sim):
    """With the option on: the object it has with the option off plus the new keys with nothing counted -- the kernel included."""
    import stream_dyn_cases as D
    import stream_input_cases as I
    import stream_loop_cases as L
    older = [(I.gain_tree(2, 128), 2, I.OPTION, 3), (L.case("comb_5_2x128")["build"](), 2, L.OPTION, 1), (D.case("knob")["build"](), 2, D.INPUTS, 2)]
    for tree, n_rows, options, n_in in older:
        a = plan_of(sim, tree, n_rows, options, n_in)["stream"]
        b = plan_of(sim, tree, n_rows, dict(options, FR_STREAM_HISTORY="1"), n_in)["stream"]
        assert a["servable"] is True and not any(k in a for k in H.NEW_KEYS), a
        stripped = {k: v for k, v in b.items() if k not in H.NEW_KEYS}
        assert stripped == a and list(stripped) == list(a)
        assert b["hist_reads"] == 0 and b["hist_dyn_reads"] == 0 and b["input_lookback"] == 0 and b["kernel"] != H.NEW_KERNEL, b


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_STREAM_HISTORY" not in r.options()
    with Renderer(sim, options=H.OPTION) as r:
        assert r.options()["FR_STREAM_HISTORY"] == {"value": "1", "source": "option"}
    clean_env.setenv("FR_STREAM_HISTORY", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_STREAM_HISTORY"] == {"value": "1", "source": "env"}
        assert "FR_STREAM_PROGRAMS" not in r.options()
    with Renderer(sim, options={"FR_STREAM_HISTORY": "0"}) as r:      # the option beats the environment
        assert r.options()["FR_STREAM_HISTORY"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_STREAM_HISTORY", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_STREAM_HISTORY": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_STREAM_HISTORY", bad)                    # the environment is read as strictly
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


def test_inert_without_stream_programs(sim, trees):
    tree = trees["gate_100"]
    assert "stream" not in plan_of(sim, tree, 2, {"FR_STREAM_HISTORY": "1"}, 2)
    said = []
    for options in ({"FR_STREAM_HISTORY": "1"}, {}):                  # the plain path's refusal, word for word what a renderer without options says
        with Renderer(sim, options=options) as r:
            synth.install(r, tree)
            with pytest.raises(RenderError) as ei:
                r.stream_begin(2)
            assert ei.value.status == FR_ERR_UNSUPPORTED
            said.append(str(ei.value))
    assert said[0] == said[1]


# ---- the dense reference and the inputs, before any GPU run -----------------------------------------------------------------------

def test_the_sequence_is_the_one_described():
    for c in H.SERVABLE:
        streams = H.streams_of(c)
        assert [len(b) for b in streams] == [12, 4] and H.frames_of(c) == 572
        assert [T for _, T, _ in streams[0][:8]] == list(K.FIRST_LENGTHS) + [5]
        assert [[idx for idx, _, _ in b] for b in streams][1][0] == 0 and streams[0][8][0] == 5003 and streams[0][10][0] == 69
        assert all(len(rows) == c["n_in"] and all(len(r) == T for r in rows) for b in streams for _, T, rows in b)
    amounts = np.concatenate([rows[2] for b in H.streams_of(H.case("knob_input")) for _, _, rows in b])
    assert (amounts < 0).any() and (amounts == 0).any() and np.isnan(amounts).any() and (amounts > H.D.KNOB_BOUND).any() and np.isinf(amounts).any()
    assert ((amounts > 0) & (amounts < H.D.KNOB_BOUND)).mean() > 0.3


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_equals_the_simulator(sim, name):
    c = H.case(name)
    tree, streams, expected = H.reference_of(name)
    n = 0
    for s, (blocks, exp) in enumerate(zip(streams, expected)):
        with Renderer(sim, semantics=c["semantics"]) as f:
            synth.install(f, tree)
            for k, ((idx, T, rows), e) in enumerate(zip(blocks, exp)):
                got = f.fill_buffer(c["n_rows"], idx, idx + T, rows)
                assert not SR.first_diff(got, e, f"{name} stream {s} block {k} at frame {idx} (T={T}), fr_fill_buffer against the reference")
                n += T
    assert n == H.frames_of(c)


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_equals_the_oracle(oracle_lib, name):
    c = H.case(name)
    tree, streams, expected = H.reference_of(name)
    n = 0
    with Renderer(oracle_lib, semantics=c["semantics"]) as o:
        synth.install(o, tree)
        for k, ((idx, T, rows), e) in enumerate(zip(streams[0], expected[0])):
            T = min(T, c["oracle_frames"] - idx)
            if T <= 0:
                break
            got = o.fill_buffer(c["n_rows"], idx, idx + T, [r[:T] for r in rows])
            assert not SR.first_diff(got, e[:, :T], f"{name} block {k} at frame {idx} (T={T}), the oracle against the reference")
            n += T
    assert n == c["oracle_frames"] > 0


@pytest.mark.parametrize("name", NAMES)
def test_every_row_is_mostly_finite(name):
    _, _, expected = H.reference_of(name)
    share = SR.finite_share([a for exp in expected for a in exp])
    print(f"{name}: finite share per row {np.round(share, 4)}")
    assert (share >= H.FINITE_SHARE).all(), share
    assert max(float(np.abs(np.where(np.isfinite(a), a, 0)).max()) for exp in expected for a in exp) > 0.01


@pytest.mark.parametrize("name", [c["name"] for c in H.SERVABLE if c["delay_rows"]])
def test_a_delay_one_frame_off_shows(name):
    c = H.case(name)
    tree, streams, expected = H.reference_of(name)
    assert SR.rows_behind_constant_delays(tree) == c["delay_rows"]
    first = [streams[0][k] for k in SR.segments_of(streams[0])[0]]       # the first segment's blocks
    ref = np.concatenate(expected[0][:len(first)], axis=1)
    off = np.concatenate(SR.expected_blocks(SR.with_delays_raised(tree), first, c["semantics"]), axis=1)
    past = int(SR.constant_delays(tree).max()) + 1
    assert past + 100 <= ref.shape[1]
    for r in c["delay_rows"]:
        a, b = ref[r, past:], off[r, past:]
        finite = np.isfinite(a)
        differ = (a.view(np.uint32) != b.view(np.uint32))[finite].mean()
        print(f"{name} row {r}: {differ:.4f} of {finite.sum()} finite samples differ with every constant delay one frame longer")
        assert differ >= H.SENSITIVITY, (r, differ)


def test_the_store_rules_sequence(sim):
    """The blocks of the GPU test of the store's rules: fr_fill_buffer of the rows as they are fed equals the dense reference
    of the rows as streamrows.hpp says the slot read them."""
    tree = H.case("gate_65")["build"]()
    fed, read = H.store_rule_blocks(np.random.default_rng(65), 65)
    exp = SR.expected_blocks(tree, read)
    with Renderer(sim) as f:
        synth.install(f, tree)
        for k, ((idx, T, rows), e) in enumerate(zip(fed, exp)):
            assert not SR.first_diff(f.fill_buffer(2, idx, idx + T, rows), e, f"block {k} at frame {idx}")
    assert all(np.abs(e).max() > 0.01 for e in exp[2:])
