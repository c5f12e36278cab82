"""FR_STREAM_EFFECTS on the CPU: the serving rule of block streaming for patches without a voice (csrc/streamplan.hpp) through the
engine's own host code in the host-logic simulator, and the proof of what tests/test_hip_stream_fx.py then relies on.
  * With FR_STREAM_PROGRAMS and FR_STREAM_EFFECTS on, every case of tests/stream_fx_cases.py is served: fr_plan_json's "stream"
    has no voice, counts the segments and the programs of each, the bus programs, the loops' strides and the delayed reads of input
    rows, and names the kernel; what stays refused says so, word for word; with the option absent or 0 every answer is what it
    is without the key, for a patch with voices and for one without.
  * The dense reference (tests/stream_reference.py) equals the simulator's fr_fill_buffer of every block of every case, and the
    C++ oracle over the first segment (a patch without a voice costs the oracle a few nodes per frame: its budget reaches all
    300 frames).
  * Conditions on the chosen inputs: every output row of the reference is at least 95 % finite, and raising every constant
    Delay by one frame changes at least 90 % of the finite samples of every row behind a delay.
The simulator has no resident launches: the kernel itself is tests/test_hip_stream_fx.py; the rule on hand-built plans, the
launch rule, the launch check and a host model of a segment's block are tests/test_stream_fx_host.py."""
import json

import numpy as np
import pytest

import sim_tools
import stream_fx_cases as F
import stream_input_cases as I
import stream_loop_cases as L
import stream_reference as SR
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, FR_ERR_UNSUPPORTED, RenderError, Renderer

NAMES = [c["name"] for c in F.SERVABLE]


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture(scope="module")
def trees():
    """Every case's graph, built once."""
    t = {c["name"]: c["build"]() for c in F.SERVABLE}
    t.update({c[0]: c[1]() for c in F.REFUSED})
    return t


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_STREAM_PROGRAMS", "FR_STREAM_BUS", "FR_STREAM_INPUTS", "FR_STREAM_BANKS", "FR_STREAM_LOOPS", "FR_STREAM_GENERAL", "FR_STREAM_DYN",
              "FR_STREAM_HISTORY", "FR_STREAM_EFFECTS", "FR_LOOP_TILES", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"):
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
        assert ("FR_STREAM_EFFECTS" in r.options()) == ("FR_STREAM_EFFECTS" in options)
        return stream_json(r) if raw else r.plan()


@pytest.mark.parametrize("name", NAMES)
def test_servable_with_the_option(sim, trees, name):
    c = F.case(name)
    s = plan_of(sim, trees[name], c["n_rows"], c["options"], c["n_in"])["stream"]
    F.check_stream_object(s, c)
    with Renderer(sim, options=c["options"]) as r:   # fr_stream_begin builds the tables (the simulator launches nothing)
        synth.install(r, trees[name])
        r.stream_begin(c["n_rows"])
        with pytest.raises(RenderError):
            r.stream_block_rows(0, [synth.time_ramp(0, 8)] * len(s["input_slots"]))
        r.fill_buffer(c["n_rows"], 0, 16, [synth.time_ramp(0, 16)] * c["n_in"])


@pytest.mark.parametrize("name", [c[0] for c in F.REFUSED])
def test_refused(sim, trees, name):
    _, _, n_rows, options, n_in, why = F.refused(name)
    s = plan_of(sim, trees[name], n_rows, options, n_in)["stream"]
    assert s["servable"] is False and s["reason"] == why, s
    assert s["kernel"] != F.NEW_KERNEL and all(k in s for k in F.NEW_KEYS) == ("FR_STREAM_EFFECTS" in options)
    with Renderer(sim, options=options) as r:
        synth.install(r, trees[name])
        with pytest.raises(RenderError) as ei:
            r.stream_begin(n_rows)
        assert ei.value.status == FR_ERR_UNSUPPORTED and why in str(ei.value)
        r.fill_buffer(n_rows, 64, 80, [synth.time_ramp(64, 80)] + [np.ones(16, np.float32)] * (n_in - 1))


def _voiced():
    """Patches with voices, each with the options that serve it."""
    return [("gain_2x128", I.gain_tree(2, 128), 2, I.OPTION, 3), ("comb_5_2x128", L.case("comb_5_2x128")["build"](), 2, L.OPTION, 1)]


@pytest.mark.parametrize("off", [None, "0"])
def test_without_the_option_every_answer_is_today_s(sim, trees, off):
    """The option absent, and "0": the text of fr_plan_json's "stream" object is, byte for byte, what a renderer that never heard
    of the option gives -- for patches with voices and for every patch without one (a refusal with today's sentence)."""
    patches = _voiced() + [(c["name"], trees[c["name"]], c["n_rows"], c["options"], c["n_in"]) for c in F.SERVABLE]
    for name, tree, n_rows, options, n_in in patches:
        plain = plan_of(sim, tree, n_rows, F.without(options, "FR_STREAM_EFFECTS"), n_in, raw=True)
        got = plan_of(sim, tree, n_rows, F.without(options, "FR_STREAM_EFFECTS") if off is None else dict(options, FR_STREAM_EFFECTS=off), n_in, raw=True)
        assert got == plain and '"stream":{' in got, name
        assert '"segments"' not in got and F.NEW_KERNEL not in got, name
        if name in NAMES:
            assert F.OLD_REASON in got and '"servable":false' in got, name


def test_a_plan_with_voices_keeps_its_stream_object(sim):
    """With the option on: the object it has with the option off plus "segments": 0 -- the kernel included."""
    for name, tree, n_rows, options, n_in in _voiced():
        a = plan_of(sim, tree, n_rows, options, n_in)["stream"]
        b = plan_of(sim, tree, n_rows, dict(options, FR_STREAM_EFFECTS="1"), n_in)["stream"]
        assert a["servable"] is True and "segments" not in a, a
        stripped = {k: v for k, v in b.items() if k not in F.NEW_KEYS}
        assert stripped == a and list(stripped) == list(a), name
        assert b["segments"] == 0 and b["kernel"] != F.NEW_KERNEL, b


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_STREAM_EFFECTS" not in r.options()
    with Renderer(sim, options=F.OPTION) as r:
        assert r.options()["FR_STREAM_EFFECTS"] == {"value": "1", "source": "option"}
    clean_env.setenv("FR_STREAM_EFFECTS", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_STREAM_EFFECTS"] == {"value": "1", "source": "env"}
        assert "FR_STREAM_PROGRAMS" not in r.options()
    with Renderer(sim, options={"FR_STREAM_EFFECTS": "0"}) as r:      # the option beats the environment
        assert r.options()["FR_STREAM_EFFECTS"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_STREAM_EFFECTS", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_STREAM_EFFECTS": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_STREAM_EFFECTS", bad)                    # the environment is read as strictly
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


def test_inert_without_stream_programs(sim, trees):
    tree = trees["echo_100"]
    assert "stream" not in plan_of(sim, tree, 1, {"FR_STREAM_EFFECTS": "1"}, 2)
    said = []
    for options in ({"FR_STREAM_EFFECTS": "1"}, {}):                  # the plain path's refusal, word for word what a renderer without options says
        with Renderer(sim, options=options) as r:
            synth.install(r, tree)
            with pytest.raises(RenderError) as ei:
                r.stream_begin(1)
            assert ei.value.status == FR_ERR_UNSUPPORTED
            said.append(str(ei.value))
    assert said[0] == said[1]


# ---- the dense reference and the inputs, before any GPU run -----------------------------------------------------------------------

def test_the_sequence_is_the_one_described():
    import stream_cases as K
    for c in F.SERVABLE:
        streams = F.streams_of(c)
        assert [len(b) for b in streams] == [12, 4] and F.frames_of(c) == 572
        assert [T for _, T, _ in streams[0][:8]] == list(K.FIRST_LENGTHS) + [5]
        assert [[idx for idx, _, _ in b] for b in streams][1][0] == 0 and streams[0][8][0] == 5003 and streams[0][10][0] == 69
        assert all(len(rows) == c["n_in"] and all(len(r) == T for r in rows) for b in streams for _, T, rows in b)


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_equals_the_simulator(sim, name):
    c = F.case(name)
    tree, streams, expected = F.reference_of(name)
    n = 0
    for s, (blocks, exp) in enumerate(zip(streams, expected)):
        with Renderer(sim) as f:
            synth.install(f, tree)
            for k, ((idx, T, rows), e) in enumerate(zip(blocks, exp)):
                got = f.fill_buffer(c["n_rows"], idx, idx + T, rows)
                assert not SR.first_diff(got, e, f"{name} stream {s} block {k} at frame {idx} (T={T}), fr_fill_buffer against the reference")
                n += T
    assert n == F.frames_of(c)


@pytest.mark.parametrize("name", NAMES)
def test_the_reference_equals_the_oracle(oracle_lib, name):
    c = F.case(name)
    tree, streams, expected = F.reference_of(name)
    n = 0
    with Renderer(oracle_lib) as o:
        synth.install(o, tree)
        for k, ((idx, T, rows), e) in enumerate(zip(streams[0], expected[0])):
            T = min(T, c["oracle_frames"] - idx)
            if T <= 0:
                break
            got = o.fill_buffer(c["n_rows"], idx, idx + T, [r[:T] for r in rows])
            assert not SR.first_diff(got, e[:, :T], f"{name} block {k} at frame {idx} (T={T}), the oracle against the reference")
            n += T
    assert n == c["oracle_frames"] == 300


@pytest.mark.parametrize("name", NAMES)
def test_every_row_is_mostly_finite(name):
    _, _, expected = F.reference_of(name)
    share = SR.finite_share([a for exp in expected for a in exp])
    print(f"{name}: finite share per row, lowest {share.min():.4f}")
    assert (share >= F.FINITE_SHARE).all(), share
    whole = np.concatenate([a for exp in expected for a in exp], axis=1)
    assert (np.abs(np.where(np.isfinite(whole), whole, 0)).max(axis=1) > 0).all()        # no row of the reference is silent
    assert max(float(np.abs(np.where(np.isfinite(a), a, 0)).max()) for exp in expected for a in exp) > 0.01


@pytest.mark.parametrize("name", [c["name"] for c in F.SERVABLE if c["delay_rows"]])
def test_a_delay_one_frame_off_shows(name):
    c = F.case(name)
    tree, streams, expected = F.reference_of(name)
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
        assert differ >= F.SENSITIVITY, (r, differ)


def test_the_store_rules_sequence(sim):
    """The blocks of the GPU test of the store's rules: fr_fill_buffer of the rows as they are fed equals the dense reference
    of the rows as streamrows.hpp says the slot read them."""
    tree = F.case("echo_100")["build"]()
    fed, read = F.store_rule_blocks(np.random.default_rng(100))
    exp = SR.expected_blocks(tree, read)
    with Renderer(sim) as f:
        synth.install(f, tree)
        for k, ((idx, T, rows), e) in enumerate(zip(fed, exp)):
            assert not SR.first_diff(f.fill_buffer(1, idx, idx + T, rows), e, f"block {k} at frame {idx}")
    assert all(np.abs(e).max() > 0.01 for e in exp[2:])


def test_the_edit_sequence(sim):
    """The GPU test's edit between two streams: the second patch's reference from frame 0 equals fr_fill_buffer of a renderer that
    had the first patch installed and rendered before."""
    a, b = F.case("echo_100"), F.case("comb_5")
    _, streams_b, exp_b = F.reference_of("comb_5")
    _, streams_a, _ = F.reference_of("echo_100")
    with Renderer(sim) as f:
        synth.install(f, a["build"]())
        for idx, T, rows in streams_a[1]:
            f.fill_buffer(1, idx, idx + T, rows)
        synth.install(f, b["build"]())
        for k, ((idx, T, rows), e) in enumerate(zip(streams_b[1], exp_b[1])):
            assert not SR.first_diff(f.fill_buffer(1, idx, idx + T, rows), e, f"block {k} at frame {idx} after the edit")
