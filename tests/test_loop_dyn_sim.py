"""FR_LOOP_DYN on the CPU: the engine's own host code in the host-logic simulator (tests/sim_tools.py).

Covered here: the option's plumbing and strictness; that unset or 0 nothing changes (the FR_ERR_CYCLE sentence byte for byte, the
plan of an ordinary echo); the lowering's cut at a Delay of a signal amount, the proof, W, the levels and the launches of every
case of tests/loop_dyn_cases.py under both forms, bit for bit against the dense forward reference, which is itself pinned to
the C++ oracle; every refusal with its status and text; what FR_LOOP_TILES, FR_RING_KEEP and block streaming answer for a sweep
plan; an edit of the depth between two calls.  NOT covered: stage_sweep_kernel -- the simulator runs a sweep launch through its
plain-loop launch_stage, a sweep at a time (engine.cpp) -- which is tests/test_hip_loop_dyn.py's."""
import numpy as np
import pytest

import loop_dyn_cases as L
import loop_dyn_reference as ldr
import sim_tools
import stage_reference as sr
import stage_variants as sv
import test_hip_parity as G
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_CYCLE, FR_ERR_INVALID_ARG, FR_ERR_UNSUPPORTED, RenderError, Renderer, f32_bits


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("FR_LOOP_DYN", "FR_LOOP_TILES", "FR_RING_KEEP", "FR_STAGE_JIT", "FR_STREAM_PROGRAMS"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


_REF = {}


def reference_for(case):
    """The case's calls with their rows and the dense forward reference's rows, computed once per process."""
    if case["key"] not in _REF:
        g = L.build(case)
        rng = np.random.default_rng(11)
        store = sr.InputStore()
        ref = ldr.DenseForward(g, case["semantics"])
        calls = []
        for what, idx, n in L.CALLS:
            rows = L.rows_for(case, what, idx, n, rng)
            store.call(idx, rows)
            exp = ref(store, idx, idx + n)
            exp.setflags(write=False)
            calls.append((what, idx, n, rows, exp))
        _REF[case["key"]] = (g, calls)
    return _REF[case["key"]]


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_LOOP_DYN" not in r.options()
    for v in ("0", "1", "2"):
        with Renderer(sim, options={"FR_LOOP_DYN": v}) as r:
            assert r.options()["FR_LOOP_DYN"] == {"value": v, "source": "option"}
    clean_env.setenv("FR_LOOP_DYN", "2")
    with Renderer(sim) as r:
        assert r.options()["FR_LOOP_DYN"] == {"value": "2", "source": "env"}
    with Renderer(sim, options={"FR_LOOP_DYN": "0"}) as r:          # the option beats the environment
        assert r.options()["FR_LOOP_DYN"] == {"value": "0", "source": "option"}
    for bad in ("3", "on", "", "-1"):
        clean_env.delenv("FR_LOOP_DYN", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_LOOP_DYN": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_LOOP_DYN", bad)
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


@pytest.mark.parametrize("opts", [{}, {"FR_LOOP_DYN": "0"}], ids=["unset", "0"])
def test_unset_or_zero_keeps_the_old_refusal_byte_for_byte(sim, clean_env, opts):
    g = L.flanger(8.0)
    with Renderer(sim, options=opts) as r:
        g.install(r)
        with pytest.raises(RenderError) as ei:
            r.fill_buffer(1, 0, 8, [np.ones(8, np.float32)] * 2)
    assert ei.value.status == FR_ERR_CYCLE
    assert str(ei.value).endswith("dependency cycle through node 2" + L.OLD_CYCLE_TEXT), str(ei.value)


def test_plan_json_of_an_ordinary_echo(sim, clean_env):
    g = sv.echo((5,))
    x = [np.arange(32, dtype=np.float32), np.zeros(32, np.float32)]
    plans = {}
    for name, opts in (("unset", {}), ("0", {"FR_LOOP_DYN": "0"}), ("1", L.SWEEP), ("2", L.WINDOWS)):
        with Renderer(sim, options={**opts, "FR_STAGE_JIT": "0"}) as r:
            g.install(r)
            r.fill_buffer(1, 0, 32, x)
            plans[name] = r.plan()
    assert "loop_dyn" not in plans["unset"]
    assert plans["0"]["loop_dyn"] == {"sweep": 0, "frames": 0, "form": "", "reason": "FR_LOOP_DYN is off"}
    for k in ("1", "2"):     # a loop of a constant delay is no sweep plan: it runs strided as ever
        assert plans[k]["loop_dyn"] == {"sweep": 0, "frames": 0, "form": "", "reason": "no loop delays by a signal amount: the strided form serves the plan"}
    drop = ("loop_dyn", "build_ms", "lower_ms", "jit_compile_ms")
    strip = lambda p: {k: v for k, v in p.items() if k not in drop}   # noqa: E731
    for k in ("0", "1", "2"):
        assert strip(plans["unset"]) == strip(plans[k]), k


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_reference_is_the_oracle(oracle_lib, case):
    """The dense forward reference against the C++ oracle, bit for bit, on every one of the first frames of the first call."""
    g, calls = reference_for(case)
    what, idx, n, rows, exp = calls[0]
    m = case["oracle"]
    with Renderer(oracle_lib, semantics=case["semantics"]) as o:
        g.install(o)
        got = o.fill_buffer(g.n_out, 0, m, [r[:m] for r in rows])
    msg = sr.first_diff(exp[:, :m], got, f"{case['key']}: dense forward reference vs the oracle on frames 0..{m - 1}")
    assert not msg, msg


@pytest.mark.parametrize("option", [1, 2], ids=["sweep", "windows"])
@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_case_on_the_simulator(sim, clean_env, case, option):
    g, calls = reference_for(case)
    with Renderer(sim, options={"FR_LOOP_DYN": str(option)}, semantics=case["semantics"]) as r:
        g.install(r)
        for what, idx, n, rows, exp in calls:
            got = r.fill_buffer(g.n_out, idx, idx + n, rows)
            plan = r.plan()
            L.check_plan(case, plan, option)
            L.check_launches(case, plan, option, what, n)
            msg = sr.first_diff(got, exp, f"{case['key']} {what} [FR_LOOP_DYN={option}]: vs the dense forward reference")
            assert not msg, msg


def one_loop(r, amount_edges, extra=()):
    """x(2) = in0 + Delay(3)(x, amount): the amount's edges given."""
    r.on_add_node(1, "F32Constant")
    r.on_add_node(2, "Sum2")
    r.on_add_node(3, "Delay")
    for h, kind in extra:
        r.on_add_node(h, kind)
    r.on_add_edge(0, 2, 0, 0)
    r.on_add_edge(3, 2, 0, 1)
    r.on_add_edge(2, 3, 0, 0)
    for e in amount_edges:
        r.on_add_edge(*e)
    r.on_add_edge(2, 0, 0, 0)


def refused(sim, build, **kw):
    with Renderer(sim, **kw) as r:
        build(r)
        with pytest.raises(RenderError) as ei:
            r.fill_buffer(1, 0, 8, [np.ones(8, np.float32), np.full(8, 2.0, np.float32)])
    return ei.value.status, str(ei.value)


@pytest.mark.parametrize("option", ["1", "2"])
def test_refusals(sim, clean_env, option):
    opts = {"FR_LOOP_DYN": option}
    # the amount is a raw input row: no bound at all, and possibly NaN
    st, msg = refused(sim, lambda r: one_loop(r, [(0, 3, 1, 1)]), options=opts)
    assert st == FR_ERR_CYCLE and "proven to lie in [-inf, inf] or to be NaN" in msg and "proven >= 1 frame" in msg and "never NaN" in msg, msg
    # 1 + lfo: the widened interval's lower end is below 1
    st, msg = refused(sim, lambda r: L.flanger(1.0, 3.0).install(r), options=opts)
    assert st == FR_ERR_CYCLE and "lowered node" in msg and "proven to lie in [0.9999" in msg and "NaN]" not in msg.split(":")[2], msg
    # bounded, >= 1, but possibly NaN: 4 + Modulo(in1, 3) without the Minimum
    st, msg = refused(sim, lambda r: one_loop(r, [(4, 3, 0, 1), (1, 4, f32_bits(4.0), 0), (5, 4, 0, 1), (0, 5, 1, 0), (1, 5, f32_bits(3.0), 1)],
                                              extra=((4, "Sum2"), (5, "Modulo"))), options=opts)
    assert st == FR_ERR_CYCLE and "or to be NaN" in msg and "[3.9999" in msg, msg
    # a signal tap of its own ring that may reach 0 frames back, next to a constant cut: today's sentence
    def own_tap(r):
        g = sr.Graph()
        x = g.node("Sum2")
        tap = g.op("Delay", x, g.op("Multiply", ("c", 3.0), L.lfo(g)))      # in [0, 3]: on the loop, in series with the constant cut
        g.connect(("in", 0), x, 0)
        g.connect(g.op("Multiply", g.op("Delay", tap, ("c", 5.0)), ("c", 0.4)), x, 1)
        g.output(x, 0)
        g.install(r)
    st, msg = refused(sim, own_tap, options=opts)
    assert st == FR_ERR_UNSUPPORTED and msg.endswith(L.OWN_RING_TEXT), msg
    # a cycle entered through the Delay's amount: that recursion never ends
    def through_amount(r):
        r.on_add_node(1, "F32Constant")
        r.on_add_node(2, "Sum2")
        r.on_add_node(3, "Delay")
        r.on_add_edge(0, 2, 0, 0)
        r.on_add_edge(3, 2, 0, 1)
        r.on_add_edge(0, 3, 0, 0)
        r.on_add_edge(2, 3, 0, 1)
        r.on_add_edge(2, 0, 0, 0)
    st, msg = refused(sim, through_amount, options=opts)
    assert st == FR_ERR_CYCLE and msg.endswith("dependency cycle through node 2" + L.OLD_CYCLE_TEXT), msg
    # no Delay at all, and a constant Delay of less than a frame
    def no_delay(r):
        r.on_add_node(2, "Sum2")
        r.on_add_node(3, "Multiply")
        r.on_add_edge(0, 2, 0, 0)
        r.on_add_edge(3, 2, 0, 1)
        r.on_add_edge(2, 3, 0, 0)
        r.on_add_edge(0, 3, 1, 1)
        r.on_add_edge(2, 0, 0, 0)
    st, msg = refused(sim, no_delay, options=opts)
    assert st == FR_ERR_CYCLE and msg.endswith(L.OLD_CYCLE_TEXT), msg
    st, msg = refused(sim, lambda r: one_loop(r, [(1, 3, f32_bits(0.5), 1)]), options=opts)
    assert st == FR_ERR_CYCLE and msg.endswith(L.OLD_CYCLE_TEXT), msg
    # what every feedback plan is refused for
    st, msg = refused(sim, lambda r: L.flanger(8.0).install(r), options=opts, mode="pull")
    assert st == FR_ERR_UNSUPPORTED and msg.endswith("a feedback loop needs the staged evaluator and contains something it cannot take "
                                                     "(a Delay by an unbounded signal or by 2^31 frames or more, or FR_MODE_PULL)"), msg
    st, msg = refused(sim, lambda r: L.flanger(8.0).install(r), options=opts, history_frames=100)
    assert st == FR_ERR_UNSUPPORTED and msg.endswith("feedback through Delay needs the full input history (fr_config.history_frames = 0)"), msg


def test_the_existing_refusal_test_with_the_option_in_the_environment(sim, clean_env):
    clean_env.setenv("FR_LOOP_DYN", "1")
    G.test_feedback_that_cannot_be_evaluated_is_refused(sim)


def test_interplay(sim, clean_env):
    g = L.flanger(8.0)
    x = [np.ones(64, np.float32), np.arange(64, dtype=np.float32)]
    with Renderer(sim, options={**L.SWEEP, "FR_LOOP_TILES": "1", "FR_RING_KEEP": "1", "FR_STREAM_PROGRAMS": "1"}) as r:
        g.install(r)
        r.fill_buffer(1, 0, 64, x)
        p = r.plan()
    assert p["loop_dyn"]["sweep"] == 7 and p["loop_dyn"]["form"] == "sweep", p["loop_dyn"]
    assert p["loop_tiles"]["frames"] == 0 and "delays by a signal amount" in p["loop_tiles"]["reason"], p["loop_tiles"]
    assert p["ring_state"]["inert"] == "a loop delays by a signal amount", p["ring_state"]
    assert not p["stream"]["servable"] and "a sweep plan, FR_LOOP_DYN" in p["stream"]["reason"], p["stream"]
    assert [l["variant"] for l in p["stage_launches"]] == ["stage_sweep_kernel/feedback+sweep"], p["stage_launches"]


@pytest.mark.parametrize("option", ["1", "2"])
def test_editing_the_depth_between_two_calls(sim, clean_env, option):
    """The depth constant 6 -> 3 after two calls: what follows is what a fresh renderer of the edited graph gives after a seek to
    the same frame (a feedback plan's rings are replayed from 0 with the inputs the store holds)."""
    rng = np.random.default_rng(3)
    rows = [L.rows_for(L.CASES[1], "steady", i * 500, 500, rng) for i in range(3)]
    g_old, g_new = L.flanger(8.0, 6.0), L.flanger(8.0, 3.0)
    depth_edge = next(e for e in g_old.edges if e[0] == 1 and e[2] == f32_bits(6.0))
    with Renderer(sim, options={"FR_LOOP_DYN": option}) as r, Renderer(sim, options={"FR_LOOP_DYN": option}) as fresh:
        g_old.install(r)
        for i in range(2):
            r.fill_buffer(1, i * 500, (i + 1) * 500, rows[i])
        r.on_del_edge(*depth_edge)
        r.on_add_edge(1, depth_edge[1], f32_bits(3.0), depth_edge[3])
        got = r.fill_buffer(1, 1000, 1500, rows[2])
        assert r.plan()["loop_dyn"]["sweep"] == 7
        g_new.install(fresh)
        for i in range(2):           # the same stored inputs, then the same call
            fresh.fill_buffer(1, i * 500, (i + 1) * 500, rows[i])
        exp = fresh.fill_buffer(1, 1000, 1500, rows[2])
    msg = sr.first_diff(got, exp, "after the edit vs a fresh renderer of the edited graph")
    assert not msg, msg
    store = sr.InputStore()
    for i in range(3):
        store.call(i * 500, rows[i])
    msg = sr.first_diff(got, ldr.render(g_new, store.rows, 1000, 1500), "after the edit vs the dense forward reference of the edited graph")
    assert not msg, msg


@pytest.mark.parametrize("option", [1, 2], ids=["sweep", "windows"])
def test_bank_case_on_the_simulator(sim, oracle_lib, clean_env, option):
    """synth.feedback_flanger, 3 voices x 64 partials: the bank fills its ring, then the sweep runs.  Every call of L.CALLS, the
    hostile time row included, on every sample against the composed reference (the oracle's voices, the dense forward loops),
    which L.bank_reference pins to the oracle's rendering of the whole tree on the first 600 frames; those frames again here."""
    tree, calls, oracle = L.bank_reference(oracle_lib)
    V = L.BANK["V"]
    with Renderer(sim, options={"FR_LOOP_DYN": str(option)}) as r:
        synth.install(r, tree)
        for what, idx, n, rows, exp in calls:
            got = r.fill_buffer(V, idx, idx + n, rows)
            p = r.plan()
            assert len(p["banks"]) == 1 and p["banks"][0]["to_ring"] and p["bank_launches"] and p["feedback_loops"] == V, p
            L.check_plan(L.BANK, p, option)
            L.check_launches(L.BANK, p, option, what, n)
            msg = sr.first_diff(got, exp, f"{L.BANK['key']} {what} [FR_LOOP_DYN={option}]: vs the oracle's voices through the dense forward loops")
            assert not msg, msg
            if what == "first":
                msg = sr.first_diff(got[:, :len(oracle[0])], oracle, f"{L.BANK['key']} [FR_LOOP_DYN={option}]: vs the oracle on the first frames")
                assert not msg, msg
