"""FR_LOOP_DYN (csrc/callplan.hpp loop_sweep): feedback through Delays of a signal amount -- the graphs, what the planner must
answer for each, and the calls every case is rendered with (plain data and graph recipes: importable without a GPU).

The amounts are built the way a host makes an LFO provable: lfo = Minimum(C(1), Modulo(in1 * rate, 1)) -- the constant on the
LEFT of Minimum keeps the amount free of NaN in both semantics whatever the row holds -- and amount = base + depth * lfo.  The
planner's interval for it is widened outward, so the proven lower bound of base + depth * lfo is floor(base) - 1 for a whole
`base` (7 for the flanger of base 8) and floor(base) for base = k + 0.5.  `W` is what fr_plan_json's loop_dyn.sweep must say;
`oracle`: the frames of the first call on which the C++ oracle pins the reference (its recursion is exponential in the frame
where a loop has two reads of itself: 48 there, 600 else).

tests/test_loop_dyn_sim.py runs the cases on the host-logic simulator, tests/test_hip_loop_dyn.py on the MI355X.
"""
import numpy as np

import stage_variants as sv
from stage_reference import Graph

FB_CHUNK = sv.FB_CHUNK
SWEEP = {"FR_LOOP_DYN": "1"}
WINDOWS = {"FR_LOOP_DYN": "2"}
OLD_CYCLE_TEXT = " with no Delay of a constant >= 1 frames on it (the reference would recurse forever)"
OWN_RING_TEXT = "a feedback plan reads a program's ring through a signal-dependent Delay"


def lfo(g, rate=0.01, slot=1):
    return g.op("Minimum", ("c", 1.0), g.op("Modulo", g.op("Multiply", ("in", slot), ("c", rate)), ("c", 1.0)))


def amount(g, base, depth, rate=0.01, slot=1):
    return g.op("Sum2", ("c", base), g.op("Multiply", ("c", depth), lfo(g, rate, slot)))


def flanger(base, depth=6.0, gain=0.5, rate=0.01):
    """x = in0 + gain * Delay(x, base + depth * lfo(in1))"""
    g = Graph()
    x = g.node("Sum2")
    g.connect(("in", 0), x, 0)
    g.connect(g.op("Multiply", g.op("Delay", x, amount(g, base, depth, rate)), ("c", gain)), x, 1)
    g.output(x, 0)
    return g


def knob():
    """x = in0 + 0.5 * Delay(x, 3 + Minimum(5, Modulo(in1, 6))): the amount is a knob row clamped to [3, 8]."""
    g = Graph()
    x = g.node("Sum2")
    g.connect(("in", 0), x, 0)
    amt = g.op("Sum2", ("c", 3.0), g.op("Minimum", ("c", 5.0), g.op("Modulo", ("in", 1), ("c", 6.0))))
    g.connect(g.op("Multiply", g.op("Delay", x, amt), ("c", 0.5)), x, 1)
    g.output(x, 0)
    return g


def two_nodes():
    """x = in0 + Delay(y, amount in [5, 9]), y = 0.5 * Delay(x, 3): two programs in a circle, merged; W = min(4, 3) = 3."""
    g = Graph()
    x = g.node("Sum2")
    dx = g.op("Delay", x, ("c", 3.0))
    y = g.op("Multiply", dx, ("c", 0.5))
    g.connect(("in", 0), x, 0)
    g.connect(g.op("Delay", y, amount(g, 5.0, 4.0)), x, 1)
    g.output(x, 0)
    g.output(y, 1)
    return g


def second_tap():
    """x = (in0 + 0.4 * Delay(x, 5)) + 0.3 * Delay(x, amount in [2, 5]): cut at the constant Delay, a signal tap of its own ring."""
    g = Graph()
    x = g.node("Sum2")
    inner = g.op("Sum2", ("in", 0), g.op("Multiply", g.op("Delay", x, ("c", 5.0)), ("c", 0.4)))
    g.connect(inner, x, 0)
    g.connect(g.op("Multiply", g.op("Delay", x, amount(g, 2.0, 3.0)), ("c", 0.3)), x, 1)
    g.output(x, 0)
    return g


def self_modulated():
    """x = in0 + 0.5 * Delay(x, 2 + Minimum(4, Modulo(Delay(x, 3), 4.5))): the amount reads the loop itself."""
    g = Graph()
    x = g.node("Sum2")
    g.connect(("in", 0), x, 0)
    amt = g.op("Sum2", ("c", 2.0), g.op("Minimum", ("c", 4.0), g.op("Modulo", g.op("Delay", x, ("c", 3.0)), ("c", 4.5))))
    g.connect(g.op("Multiply", g.op("Delay", x, amt), ("c", 0.5)), x, 1)
    g.output(x, 0)
    return g


def tap_behind():
    """The flanger of base 8, and behind it y = in0 + Delay(x, 3 * lfo): a signal tap that may reach 0 frames back -- the next level."""
    g = Graph()
    x = g.node("Sum2")
    g.connect(("in", 0), x, 0)
    g.connect(g.op("Multiply", g.op("Delay", x, amount(g, 8.0, 6.0)), ("c", 0.5)), x, 1)
    y = g.op("Sum2", ("in", 0), g.op("Delay", x, g.op("Multiply", ("c", 3.0), lfo(g, 0.03))))
    g.output(y, 0)
    g.output(x, 1)
    return g


def many(n):
    """n independent flangers of base 8 on one amount, gains 0.2 .. 0.7: more programs than one workgroup row, grid.y."""
    g = Graph()
    amt = amount(g, 8.0, 6.0)
    for i in range(n):
        x = g.node("Sum2")
        g.connect(("in", 0), x, 0)
        g.connect(g.op("Multiply", g.op("Delay", x, amt), ("c", 0.2 + 0.5 * i / n)), x, 1)
        g.output(x, i)
    return g


GRAPHS = {"flanger": flanger, "knob": knob, "two_nodes": two_nodes, "second_tap": second_tap, "self_modulated": self_modulated,
          "tap_behind": tap_behind, "many": many}


def _case(key, graph, W, oracle=600, levels=1, semantics="reference", knob_row=False):
    return {"key": key, "graph": graph, "W": W, "oracle": oracle, "levels": levels, "semantics": semantics, "n_in": 2, "knob_row": knob_row}


CASES = [
    _case("W=1 [2,5]", ("flanger", (2.0, 3.0)), 1),
    _case("W=7 flanger", ("flanger", (8.0,)), 7),
    _case("wave edge 63", ("flanger", (64.0,)), 63),
    _case("wave edge 64", ("flanger", (64.5,)), 64),
    _case("wave edge 65", ("flanger", (65.5,)), 65),
    _case("cap edge 255", ("flanger", (256.0,)), 255),
    _case("cap edge 256", ("flanger", (256.5,)), 256),
    _case("cap edge 257", ("flanger", (257.5,)), 257),
    _case("cap edge 300", ("flanger", (300.5,)), 300),
    _case("knob row", ("knob", ()), 2, knob_row=True),
    _case("two merged nodes", ("two_nodes", ()), 3),
    _case("constant cut, signal tap", ("second_tap", ()), 1, oracle=48),
    _case("self-modulated", ("self_modulated", ()), 1, oracle=48),
    _case("tap behind the loop", ("tap_behind", ()), 7, levels=2),
    _case("300 loops", ("many", (300,)), 7),
    _case("W=7 flanger sparkle", ("flanger", (8.0,)), 7, semantics="sparkle"),
]
IDS = [c["key"] for c in CASES]

# (what, first frame, frames): first call, a ragged steady call, one frame, a short call (fr_plan_json lists 256 launches at
# most: the windows form's launches are counted here for the small W too), a seek past FB_CHUNK (the replay crosses a chunk), a
# seek back, a call that makes the rings grow and wrap, and a call whose rows -- the LFO's time row included -- are hostile
CALLS = [("first", 0, 1000), ("steady", 1000, 777), ("one frame", 1777, 1), ("short", 1778, 100), ("seek", 20000, 64), ("seek back", 300, 500),
         ("long", 800, 40000), ("hostile", 40800, 512)]
KNOB = np.array([0.0, 5.9, 5.0, 4.999, 0.25, 0.5, 1.0, 1.75, 2.5, 3.999, 4.0, 6.0, 6.5, 11.9, -0.25, -6.0, 3.0, 0.999], np.float32)


def build(case):
    name, args = case["graph"]
    return GRAPHS[name](*args)


def rows_for(case, what, idx, n, rng):
    """in0: noise; in1: the frame ramp the LFOs read (a knob row for the knob case).  The hostile call: NaN, infinities, -0,
    subnormals and huge values in BOTH rows -- the proof, not the data, keeps the amount in its range."""
    in0 = (rng.normal(size=n) * 3).astype(np.float32)
    in1 = np.arange(idx, idx + n, dtype=np.float64).astype(np.float32)
    if case["knob_row"]:
        in1 = np.resize(KNOB, n).astype(np.float32)
        in1[::7] = (rng.random(len(in1[::7])) * 12 - 3).astype(np.float32)
    if what == "hostile":
        in0[::5] = np.resize(sv.HOSTILE, len(in0[::5]))
        in1[1::3] = np.resize(sv.HOSTILE, len(in1[1::3]))
    return [in0, in1]


# ---- the bank case: 3 voices x 64 partials through the flanger (libfriendship_amd.synth.feedback_flanger) ----------------------
# The bank fills its ring, then the sweep runs.  Its reference is composed: the voices are functions of the time row at the same
# frame alone, so the ORACLE renders them (bank_voice_tree: the same partials without the loops) call by call, and the dense
# forward reference runs the loops on those rows -- BANK_LOOPS, the flanger of every voice with the voice as an input row.  (The
# dense reference on the whole tree would hold a row per node: 2000 nodes x 41 000 frames.)  The whole tree is pinned to the oracle
# on the first 600 frames like every single-tap case.
BANK = {"key": "3 voices x 64 partials", "V": 3, "P": 64, "base": 8.0, "depth": 6.0, "rate": 0.01, "gain": 0.5, "W": 7, "oracle": 600,
        "levels": 1, "n_in": 1, "knob_row": False}


def bank_tree():
    from libfriendship_amd import synth
    b = BANK
    return synth.feedback_flanger(b["V"], b["P"], b["base"], b["depth"], b["rate"], b["gain"])


def bank_voice_tree():
    """The voices of bank_tree() alone, one per output row: same parameters, same leaves, same sum tree."""
    from libfriendship_amd import synth
    b = BANK
    p = synth.voice_params(b["V"], b["P"], 0x5EED0300, wrap=64)
    g = synth.GraphArrays()
    voice = synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"], 0).reshape(b["V"], b["P"]))
    g.edge(voice, 0, 0, np.arange(b["V"], dtype=np.uint32))
    return g.finish(b["V"])


def bank_loops():
    """x_v = in[1 + v] + gain * Delay(x_v, base + depth * Minimum(1, Modulo(in0 * rate_v, 1))): feedback_flanger's loops, node for node."""
    b = BANK
    rates = (np.float32(b["rate"]) * np.arange(1, b["V"] + 1, dtype=np.float32)).astype(np.float32)
    g = Graph()
    for v in range(b["V"]):
        ramp = g.op("Modulo", g.op("Multiply", ("in", 0), ("c", rates[v])), ("c", 1.0))
        amt = g.op("Sum2", ("c", b["base"]), g.op("Multiply", ("c", b["depth"]), g.op("Minimum", ("c", 1.0), ramp)))
        x = g.node("Sum2")
        g.connect(("in", 1 + v), x, 0)
        g.connect(g.op("Multiply", g.op("Delay", x, amt), ("c", b["gain"])), x, 1)
        g.output(x, v)
    return g


def bank_time_row(what, idx, n):
    t = np.arange(idx, idx + n, dtype=np.float64).astype(np.float32)
    if what == "hostile":
        t[1::3] = np.resize(sv.HOSTILE, len(t[1::3]))
    return t


_BANK_REF = {}


def bank_reference(oracle_lib, semantics="reference"):
    """(tree, calls, oracle): the bank case's calls as (what, idx, n, [time row], expected rows) -- the voices from the oracle, the
    loops from the dense forward reference --, computed once per process, and the oracle's rendering of the WHOLE tree on the
    first BANK["oracle"] frames, which the expected rows must equal bit for bit (asserted here: the pin)."""
    if semantics in _BANK_REF:
        return _BANK_REF[semantics]
    import loop_dyn_reference as ldr
    import stage_reference as sr
    from libfriendship_amd import synth
    from libfriendship_amd.capi import Renderer
    b = BANK
    tree, voices, loops = bank_tree(), bank_voice_tree(), bank_loops()
    store = sr.InputStore()
    ref = ldr.DenseForward(loops, semantics)
    calls = []
    for what, idx, n in CALLS:
        t = bank_time_row(what, idx, n)
        with Renderer(oracle_lib, semantics=semantics) as o:      # a voice is a function of the time row at the same frame alone
            synth.install(o, voices)
            v = o.fill_buffer(b["V"], idx, idx + n, [t])
        store.call(idx, [t] + [v[k] for k in range(b["V"])])
        exp = ref(store, idx, idx + n)
        exp.setflags(write=False)
        calls.append((what, idx, n, [t], exp))
    m = b["oracle"]
    with Renderer(oracle_lib, semantics=semantics) as o:
        synth.install(o, tree)
        oracle = o.fill_buffer(b["V"], 0, m, [calls[0][3][0][:m]])
    msg = sr.first_diff(calls[0][4][:, :m], oracle, f"{b['key']} [{semantics}]: oracle voices + dense forward loops vs the oracle on frames 0..{m - 1}")
    assert not msg, msg
    _BANK_REF[semantics] = (tree, calls, oracle)
    return _BANK_REF[semantics]


def form_of(variant):
    return variant.split("/", 1)[1]


def check_plan(case, plan, option):
    """loop_dyn of a plan rendered with FR_LOOP_DYN = option (1 or 2): W, the frames per sweep and the form."""
    ld = plan["loop_dyn"]
    assert plan["feedback"] and plan["pull_rows"] == 0 and plan["fused_stride"] == 0 and plan["stage_jit_form"] is None and not plan["stage_jit"], (case["key"], plan)
    assert ld["sweep"] == case["W"] and ld["frames"] == min(case["W"], 256) and ld["form"] == ("sweep" if option == 1 else "windows"), (case["key"], ld)
    assert plan["fused_levels"] == case["levels"], (case["key"], plan["fused_levels"])
    return ld


def check_launches(case, plan, option, what, n):
    """The launches of a call of n frames: a sweep launch per level (feedback; replay after a seek), or the windows form's
    ceil(n / W) launches of stage_kernel per level; copies stay stage_kernel/copy."""
    launches = plan["stage_launches"]
    variants = [l["variant"] for l in launches]
    steady = [v for v in variants if "replay" not in v and not v.endswith("/copy") and v != "stage_kernel/windows"]
    if option == 1:
        assert steady == ["stage_sweep_kernel/feedback+sweep"] * case["levels"], (case["key"], what, variants)
        assert all(l["stride"] == min(case["W"], 256) for l in launches if l["variant"].endswith("+sweep")), (case["key"], what, launches)
        if what in ("seek", "seek back"):
            assert "stage_sweep_kernel/replay+sweep" in variants, (case["key"], what, variants)
    else:
        assert not steady and "stage_kernel/windows" in variants, (case["key"], what, variants)
        assert not any("sweep" in v for v in variants), (case["key"], what, variants)
        if what in ("first", "steady", "one frame", "short"):                  # (fr_plan_json lists 256 launches at most)
            assert what != "short" or case["levels"] * -(-n // case["W"]) < 256, (case["key"], "the short call must be countable")
        if what in ("first", "steady", "one frame", "short") and len(launches) < 256:
            assert variants.count("stage_kernel/windows") == case["levels"] * -(-n // case["W"]), (case["key"], what, n, len(variants))
    return variants
