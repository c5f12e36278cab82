"""FR_LOOP_TILES (csrc/callplan.hpp loop_tile): the feedback cases of tests/stage_variants.py that the option tiles, the ones
it refuses with the reason fr_plan_json gives, and one recipe of its own (plain data and graph recipes: importable without
a GPU).

A case: `key` (its name), `graph` (a recipe of GRAPHS and its arguments; the argument "max" stands for the plan's
loop_tiles.max_stride, "max+1" for one more), the steady call's length `T`, the frame of the `seek` forward (past FB_CHUNK,
so the replay crosses a chunk boundary), `n_in`, the `hostile` input slot, `semantics`, and what the rule answers: `tiled`
(the strided launches of the steady call and of the replay carry +tile) or the `reason` fr_plan_json gives for frames = 0.
tests/test_loop_tiles_sim.py runs them on the host-logic simulator, tests/test_hip_loop_tiles.py on the MI355X.
"""
import importlib.util
import os

import numpy as np

import stage_reference as sr
import stage_variants as sv
from stage_reference import Graph

FB_CHUNK = sv.FB_CHUNK
ON = {"FR_LOOP_TILES": "1"}
OFF = {"FR_LOOP_TILES": "0"}


def arith_loop():
    """x = in0 + Minimum(Modulo(Divide(Multiply(Delay(x, 1), 0.5), in1), 1.5), in0): the four other primitives inside a
    one-sample loop, the second input as the divisor (hostile row: zeros, infinities, NaN, subnormals among the divisors)."""
    g = Graph()
    x = g.node("Sum2")
    g.connect(("in", 0), x, 0)
    m = g.op("Multiply", g.op("Delay", x, ("c", 1.0)), ("c", 0.5))
    q = g.op("Divide", m, ("in", 1))
    r = g.op("Modulo", q, ("c", 1.5))
    g.connect(g.op("Minimum", r, ("in", 0)), x, 1)
    g.output(x, 0)
    return g


GRAPHS = {**sv.GRAPHS, "arith_loop": arith_loop}


def _case(key, graph, T, seek, tiled=True, reason=None, n_in=2, hostile=0, semantics="reference"):
    return {"key": key, "graph": graph, "T": T, "seek": seek, "tiled": tiled, "reason": reason, "n_in": n_in, "hostile": hostile,
            "semantics": semantics}


CASES = [
    _case("echo(1)", ("echo", ((1,),)), 1000, FB_CHUNK + 1500),
    # 255 frames per tile: ragged last tiles in the call (2001 = 7 * 255 + 216) and in the replay's last chunk
    _case("echo(3)", ("echo", ((3,),)), 2001, FB_CHUNK + 77),
    _case("echo(max_stride)", ("echo", (("max",),)), 1000, FB_CHUNK + 300),
    # row copies after the strided launch, and a later level whose read of the loop's ring at delay 2 is a tile load
    _case("rows_inside(5)", ("rows_inside", (5,)), 777, FB_CHUNK + 5),
    _case("many_inputs(10, 7)", ("many_inputs", (10, 7)), 900, FB_CHUNK + 9, n_in=10),       # the input table in device memory
    _case("many_loads(8, 2)", ("many_loads", (8, 2)), 1001, FB_CHUNK + 3),                   # eight `t < d` tests in the load phase
    _case("arith_loop", ("arith_loop", ()), 700, FB_CHUNK + 11, hostile=1),
    _case("arith_loop sparkle", ("arith_loop", ()), 700, FB_CHUNK + 11, hostile=1, semantics="sparkle"),
    # not tiled: the same bits, the reason asserted
    _case("echo(max_stride + 1)", ("echo", (("max+1",),)), 1000, FB_CHUNK + 300, tiled=False, reason="the loops' stride is {max+1} frames"),
    _case("echo(2, 4)", ("echo", ((2, 4),)), 1501, FB_CHUNK + 300, tiled=False, reason="a loop reads its own ring further back than one stride"),
    _case("many_loads(17, 5)", ("many_loads", (17, 5)), 1001, FB_CHUNK + 3, tiled=False, reason="has 17 frame-only loads"),
]
IDS = [c["key"] for c in CASES]


def max_stride(lib):
    """loop_tiles.max_stride as the plan JSON of `lib` reports it."""
    from libfriendship_amd.capi import Renderer
    with Renderer(lib, options=ON) as r:
        sv.echo((1,)).install(r)
        r.fill_buffer(1, 0, 4, [np.zeros(4, np.float32), np.zeros(4, np.float32)])
        return int(r.plan()["loop_tiles"]["max_stride"])


def resolve(case, ms):
    """The case with "max" / "max+1" replaced by the plan's max_stride (+ 1)."""
    sub = {"max": ms, "max+1": ms + 1}

    def fix(a):
        if isinstance(a, tuple):
            return tuple(fix(x) for x in a)
        return sub.get(a, a) if isinstance(a, str) else a
    name, args = case["graph"]
    reason = case["reason"].replace("{max+1}", str(ms + 1)) if case["reason"] else None
    return {**case, "graph": (name, fix(args)), "reason": reason}


def build(case):
    name, args = case["graph"]
    return GRAPHS[name](*args)


def form_of(variant):
    return variant.split("/", 1)[1]


def check_launches(case, plan, what):
    """The plan of a call of `case` rendered with the option on: loop_tiles says what the case expects, every strided launch
    (feedback, replay) carries +tile exactly when the plan is tiled, no other launch does."""
    lt = plan["loop_tiles"]
    launches = plan["stage_launches"]
    assert plan["feedback"] and plan["pull_rows"] == 0 and launches, (case["key"], what, plan)
    stride = plan["fused_stride"]
    if case["tiled"]:
        assert lt["frames"] == stride * (256 // stride) and lt["reason"] == "" and 1 <= stride <= lt["max_stride"], (case["key"], lt, stride)
    else:
        assert lt["frames"] == 0 and case["reason"] in lt["reason"], (case["key"], lt)
    for l in launches:
        flags = form_of(l["variant"]).split("+")
        strided = flags[0] in ("feedback", "replay")
        assert ("tile" in flags) == (strided and case["tiled"]), (case["key"], what, l)
        if "tile" in flags:
            assert flags[1:3] == ["carry_only", "tile"] and l["stride"] == stride, (case["key"], what, l)
    forms = [form_of(l["variant"]).split("+")[0] for l in launches]
    assert "feedback" in forms, (case["key"], what, forms)
    return forms


def comb_tree(V, P, d):
    """The patch of tools/feedback_bench.py: V voices of P partials, each through x = voice + 0.6 * Delay(x, d)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "feedback_bench.py")
    spec = importlib.util.spec_from_file_location("feedback_bench", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.comb_tree(V, P, d)


__all__ = ["CASES", "IDS", "ON", "OFF", "FB_CHUNK", "GRAPHS", "arith_loop", "build", "resolve", "max_stride", "check_launches", "form_of",
           "comb_tree", "sr"]
