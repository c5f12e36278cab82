"""Every stage-program launch form the engine's rule can pick, and a small case that reaches each (plain data and graph
recipes: importable without a GPU).

A key is what fr_plan_json's "stage_launches" reports as "variant" (engine.cpp stage_variant): the kernel -- stage_kernel
(the interpreter, FR_STAGE_JIT=0) or jit_stage[plain|deep, P (MAXP > 0), defer, B<BLK>] (compiled, FR_STAGE_JIT=force) --
the launch form (levels, fused, strided, feedback, copy, replay) and the paths its arguments select (+carry, +carry_only,
+table, +grid<N>).  A case's `key` is the variant its steady call runs (the second call: contiguous, after a first call
that fills the rings); `replay` is the variant a seek of a feedback case replays with.  tests/test_stage_variants.py runs
every case on the host-logic simulator (which interprets: the part after "/" is asserted there) and checks that no key
matches UNREACHABLE; tests/test_hip_stage_matrix.py runs every case on the MI355X against the dense reference
(tests/stage_reference.py), bit for bit, and asserts the whole key.

A case: `graph` (a recipe name of GRAPHS and its arguments), the per-renderer `options`, the steady call's length `T`,
`semantics`, the entry point ("host": fill_buffer; "dense": fill_buffer_dense), `hostile` (the input slot whose row the
hostile call fills with HOSTILE values, or with HOSTILE_AMOUNTS for a Delay amount's slot) and `seek` (the frame of the seek
forward: past FB_CHUNK = 16384 for feedback cases, so the replay crosses a chunk boundary).
"""
import numpy as np

from stage_reference import Graph

FB_CHUNK = 16384
HOSTILE = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -3e-39, 1e30, -1e30, 3e38, -3e38, 0.5, -2.25], np.float32)
HOSTILE_AMOUNTS = np.array([np.nan, -0.0, -3.0, 2.5, 0.75, 18446744073709551616.0, np.inf, -np.inf, 7.0, 1e-45, 31.999998, 5.0],
                           np.float32)
BOUNDED_AMOUNTS = np.array([np.nan, -0.0, -3.0, 2.5, 0.75, -np.inf, 7.0, 1e-45, 31.999998, 5.0, -1e30], np.float32)


# ---- graph recipes ------------------------------------------------------------------------------------------------
def chain(delays, rows_every=False):
    """x_{k+1} = Delay(x_k, d_k) * c_k + Modulo(x_k, 1.5) -- a program per node, each reading the ring of the one before
    (Min(in1, .) at the head: two input slots).  Output: the last node (and every node with rows_every)."""
    g = Graph()
    x = g.op("Minimum", ("in", 0), ("in", 1))
    outs = [x]
    for k, d in enumerate(delays):
        m = g.op("Multiply", g.op("Delay", x, ("c", float(d))), ("c", 0.5 + 0.0625 * k))
        x = g.op("Sum2", m, g.op("Modulo", x, ("c", 1.5)))
        outs.append(x)
    for r, o in enumerate(outs if rows_every else [x]):
        g.output(o, r)
    return g


def echo(taps, gain=0.5):
    """x = in0 + sum_k gain_k * Delay(x, d_k): one feedback loop.  taps: the delays."""
    g = Graph()
    acc = ("in", 0)
    x = g.node("Sum2")
    g.connect(acc, x, 0)
    fb = None
    for k, d in enumerate(taps):
        t = g.op("Multiply", g.op("Delay", x, ("c", float(d))), ("c", gain / (k + 1)))
        fb = t if fb is None else g.op("Sum2", fb, t)
    g.connect(fb, x, 1)
    g.output(x, 0)
    return g


def ring_loop(n, d):
    """x_0 = in0 + Delay(x_{n-1}, d), x_k = 0.9 * Delay(x_{k-1}, d) (+ in1 mod 1.5): n delayed nodes around one loop -- merged
    into one program that stores n rings (carry slots for 8 of them).  Output: x_0 and x_{n-1}."""
    g = Graph()
    xs = [g.node("Sum2")]
    g.connect(("in", 0), xs[0], 0)
    for k in range(1, n):
        y = g.op("Multiply", g.op("Delay", xs[-1], ("c", float(d))), ("c", 0.9 - 0.01 * k))
        xs.append(g.op("Sum2", y, g.op("Modulo", ("in", 1), ("c", 1.5))) if k % 3 == 0 else y)
    g.connect(g.op("Delay", xs[-1], ("c", float(d))), xs[0], 1)
    g.output(xs[0], 0)
    g.output(xs[-1], 1)
    return g


def rows_inside(d):
    """m = x * 0.75, x = in0 + Delay(m, d), row 2 = Delay(x, 2) + in1: rows inside the loop (copy programs) and a later level."""
    g = Graph()
    x = g.node("Sum2")
    g.connect(("in", 0), x, 0)
    m = g.op("Multiply", x, ("c", 0.75))
    g.connect(g.op("Delay", m, ("c", float(d))), x, 1)
    g.output(x, 0)
    g.output(m, 1)
    g.output(g.op("Sum2", g.op("Delay", x, ("c", 2.0)), ("in", 1)), 2)
    return g


def many_loads(n_loads, d=None):
    """sum_k Modulo(Delay(in_{k%2}, k + 1), 1.5 + k / 8): n_loads delayed input reads in one program; with d, summed into the
    loop x = that + 0.5 * Delay(x, d)."""
    g = Graph()
    acc = None
    for k in range(n_loads):
        t = g.op("Modulo", g.op("Delay", ("in", k % 2), ("c", float(k + 1))), ("c", 1.5 + k / 8))
        acc = t if acc is None else g.op("Sum2", acc, t)
    if d is not None:
        x = g.node("Sum2")
        g.connect(acc, x, 0)
        g.connect(g.op("Multiply", g.op("Delay", x, ("c", float(d))), ("c", 0.5)), x, 1)
        acc = x
    g.output(acc, 0)
    return g


def delayed_reads(n_loads):
    """Delay(in_0, 1) + Delay(in_1, 2) + ... + Delay(in_{k%2}, k + 1): a program of exactly n_loads loads (no constant: the
    amounts are the reads' parameters)."""
    g = Graph()
    acc = None
    for k in range(n_loads):
        t = g.op("Delay", ("in", k % 2), ("c", float(k + 1)))
        acc = t if acc is None else g.op("Sum2", acc, t)
    g.output(acc, 0)
    return g


def many_inputs(n_in, d=None):
    """Delay(in_0, 1) + in_1 * c + ... over n_in input slots (> 8: the input table in device memory); with d, in a loop."""
    g = Graph()
    acc = g.op("Delay", ("in", 0), ("c", 1.0))
    for k in range(1, n_in):
        acc = g.op("Sum2", acc, g.op("Multiply", ("in", k), ("c", 1.0 + k / 16)))
    if d is not None:
        x = g.node("Sum2")
        g.connect(acc, x, 0)
        g.connect(g.op("Multiply", g.op("Delay", x, ("c", float(d))), ("c", 0.5)), x, 1)
        acc = x
    g.output(acc, 0)
    return g


def dyn_delays():
    """The three Delays of a signal amount: of an input (S_READ_INPUT_DYN) and of a constant (S_STEP_DYN) by in1, of a node's
    ring (S_READ_DYN) by in2; the node x = Delay(in0, 2) * 0.5 + in0 feeds the last.  Rows: each, and their sum.  (A ring's
    read needs a bound: an amount row with +inf or 2^64 -- HOSTILE_AMOUNTS -- sends it to the pull interpreter, so in2 gets
    BOUNDED_AMOUNTS.)"""
    g = Graph()
    x = g.op("Sum2", g.op("Multiply", g.op("Delay", ("in", 0), ("c", 2.0)), ("c", 0.5)), ("in", 0))
    a = g.op("Delay", x, ("in", 2))
    b = g.op("Delay", ("in", 0), ("in", 1))
    c = g.op("Delay", ("c", 3.5), ("in", 1))
    g.output(a, 0)
    g.output(b, 1)
    g.output(c, 2)
    g.output(g.op("Sum2", g.op("Sum2", a, b), c), 3)
    return g


def wide(n_rows, d=3):
    """n_rows rows c_i * Delay(in0, d): one level of n_rows programs."""
    g = Graph()
    dl = g.op("Delay", ("in", 0), ("c", float(d)))
    for r in range(n_rows):
        g.output(g.op("Multiply", dl, ("c", 1.0 + r / 65536)), r)
    return g


GRAPHS = {"chain": chain, "echo": echo, "ring_loop": ring_loop, "rows_inside": rows_inside, "many_loads": many_loads, "delayed_reads": delayed_reads,
          "many_inputs": many_inputs, "dyn_delays": dyn_delays, "wide": wide}


def build(case):
    name, args = case["graph"]
    return GRAPHS[name](*args)


def _case(key, graph, T, options=None, semantics="reference", entry="host", hostile=0, seek=None, replay=None, n_in=2,
          hoisted=None):
    return {"key": key, "graph": graph, "T": T, "options": dict(options or {}), "semantics": semantics, "entry": entry,
            "hostile": hostile, "seek": seek, "replay": replay, "n_in": n_in, "hoisted": hoisted}


_I = {"FR_STAGE_JIT": "0"}
_J = {"FR_STAGE_JIT": "force"}
_OBS = {"FR_DELAY_OBSERVED": "1"}

CASES = [
    # no feedback: a level per launch (delays below 64), sub-windows of fused_max_frames, one strided launch
    _case("stage_kernel/levels", ("chain", ((3, 5, 7, 11),)), 301, _I),
    _case("jit_stage[plain,B1]/levels", ("chain", ((3, 5, 7, 11),)), 301, _J),
    _case("stage_kernel/fused", ("chain", ((64, 65, 67, 70, 71, 73, 79),)), 333, _I),
    _case("jit_stage[plain,B1]/fused", ("chain", ((64, 65, 67, 70, 71, 73, 79),)), 333, _J),
    _case("stage_kernel/strided", ("chain", ((300, 600, 300),)), 517, _I),
    _case("stage_kernel/strided#8", ("chain", ((300, 600, 300),)), 2317, _I),
    _case("jit_stage[plain,B1]/strided", ("chain", ((300, 600, 300),)), 2317, _J),
    _case("jit_stage[plain,B1]/strided#2", ("chain", ((300, 600, 300),)), 517, _J),
    _case("jit_stage[deep,P,B4]/strided", ("chain", ((300, 600, 300),)), 517, {**_J, "FR_STAGE_BLOCK": "4"}),
    # ... FR_STAGE_STRIDED=0: the same graph and length as the fused form, the same bits
    _case("stage_kernel/fused#strided-off", ("chain", ((300, 600, 300),)), 517, {**_I, "FR_STAGE_STRIDED": "0"}),
    # feedback, every loop read through the carry
    _case("stage_kernel/feedback+carry_only", ("echo", ((1,),)), 1000, _I, seek=FB_CHUNK + 1500,
          replay="stage_kernel/replay+carry_only"),
    _case("stage_kernel/feedback+carry_only#d3", ("echo", ((3,),)), 2001, _I, seek=FB_CHUNK + 77),
    _case("stage_kernel/feedback+carry_only#d300", ("echo", ((300,),)), 5003, _I, seek=FB_CHUNK + 901),
    _case("jit_stage[deep,P,defer,B8]/feedback+carry_only", ("echo", ((1,),)), 1000, _J, seek=FB_CHUNK + 1500,
          replay="jit_stage[deep,P,defer,B8]/replay+carry_only"),
    _case("jit_stage[deep,P,defer,B8]/feedback+carry_only#d3", ("echo", ((3,),)), 2001, _J, seek=FB_CHUNK + 77),
    _case("jit_stage[deep,P,defer,B8]/feedback+carry_only#d300", ("echo", ((300,),)), 5003, _J, seek=FB_CHUNK + 901),
    _case("jit_stage[deep,P,defer,B1]/feedback+carry_only#block1", ("echo", ((3,),)), 2001, {**_J, "FR_STAGE_BLOCK": "1"},
          seek=FB_CHUNK + 77),
    # feedback with reads further back than one iteration (0xFF: through memory) -- taps at d and 2d; a merged loop of 11 rings
    _case("stage_kernel/feedback+carry", ("echo", ((2, 4),)), 1501, _I, seek=FB_CHUNK + 300, replay="stage_kernel/replay+carry"),
    _case("jit_stage[deep,P,B10]/feedback+carry", ("echo", ((2, 4),)), 1501, _J, seek=FB_CHUNK + 300,
          replay="jit_stage[deep,P,B10]/replay+carry"),
    _case("stage_kernel/feedback+carry#rings11", ("ring_loop", (11, 3)), 1201, _I, seek=FB_CHUNK + 10),
    _case("jit_stage[deep,P,B8]/feedback+carry#rings11", ("ring_loop", (11, 3)), 1201, _J, seek=FB_CHUNK + 10),
    # rows inside a loop: copy programs after the strided launch
    _case("stage_kernel/copy", ("rows_inside", (5,)), 777, _I, seek=FB_CHUNK + 5),
    _case("jit_stage[deep,P,B16]/copy", ("rows_inside", (5,)), 777, _J, seek=FB_CHUNK + 5),
    # generated forms: a parameter row of more than 64 words (34 delayed input reads, MAXP 0); 17 pure loads (over the MAXLD
    # cap of 16)
    _case("jit_stage[deep,defer,B1]/feedback+carry_only", ("many_loads", (34, 2)), 1001, _J, seek=FB_CHUNK + 3),
    _case("jit_stage[deep,P,defer,B1]/feedback+carry_only", ("many_loads", (17, 5)), 1001, _J, seek=FB_CHUNK + 3),
    # interpreter load hoisting: 24 and 25 loads in one program, constants counted (STAGE_MAX_HOISTED = 24: all 24 issued
    # back to back; 25, none -- each where it is used)
    _case("stage_kernel/levels#loads24", ("delayed_reads", (24,)), 700, _I, hoisted=24),
    _case("stage_kernel/levels#loads25", ("delayed_reads", (25,)), 700, _I, hoisted=0),
    # more than 8 input slots: the input table in device memory
    _case("stage_kernel/levels+table", ("many_inputs", (11,)), 500, _I, n_in=11),
    _case("jit_stage[plain,B1]/levels+table", ("many_inputs", (11,)), 500, _J, n_in=11),
    _case("stage_kernel/feedback+carry_only+table", ("many_inputs", (10, 7)), 900, _I, seek=FB_CHUNK + 9, n_in=10),
    _case("jit_stage[deep,P,defer,B2]/feedback+carry_only+table", ("many_inputs", (10, 7)), 900, _J, seek=FB_CHUNK + 9, n_in=10),
    # Delays of a signal amount, hostile amounts, both semantics
    _case("stage_kernel/levels#dyn", ("dyn_delays", ()), 400, {**_I, **_OBS}, hostile=1, n_in=3),
    _case("stage_kernel/levels#dyn-sparkle", ("dyn_delays", ()), 400, {**_I, **_OBS}, semantics="sparkle", hostile=1, n_in=3),
    _case("jit_stage[plain,B1]/levels#dyn", ("dyn_delays", ()), 400, {**_J, **_OBS}, hostile=1, n_in=3),
    _case("jit_stage[plain,B1]/levels#dyn-sparkle", ("dyn_delays", ()), 400, {**_J, **_OBS}, semantics="sparkle", hostile=1, n_in=3),
    # one level of more than 65535 programs: cut at the grid.y limit
    _case("stage_kernel/levels+grid2", ("wide", (66000,)), 37, _I, entry="dense", n_in=1),
    _case("jit_stage[plain,B1]/levels+grid2", ("wide", (66000,)), 37, _J, entry="dense", n_in=1),
]

# Combinations the rule never produces (a key matching one of these patterns must not appear)
UNREACHABLE = {
    "+carry on a launch that does not stride": "use_carry is set only for the strided launches of feedback plans",
    "+carry on strided (no feedback)": "without feedback use_carry stays 0: a thread's earlier strides are read through memory",
    "defer without carry_only": "plan_stage_jit defers stores only for fused_carry_only plans (DEFER needs nothing in a block "
                                "to read what it stores)",
    "a feedback launch whose carry flag is not the plan's": "a strided launch of a feedback plan always carries, and carries "
                                                            "only exactly when the plan is fused_carry_only",
    "deep in a plan without feedback unless FR_STAGE_BLOCK > 1": "the block is 1 without feedback and the deep form needs a "
                                                                "block > 1 or deferred stores",
    "replay without feedback": "only feedback plans replay history after a seek",
    "fused / strided / levels in a feedback plan": "a feedback plan always runs its strided fused levels and copy programs",
}


def key_base(key):
    """The variant a case's key names (a '#' suffix only tells cases of one key apart)."""
    return key.split("#")[0]


def unreachable(variant, feedback, block_option, carry_only=None):
    """The UNREACHABLE entry `variant` would match, or None.  feedback / carry_only: fr_plan_json's "feedback" and
    "fused_carry_only" for the plan that ran it (carry_only None: not known, those checks are skipped)."""
    kernel, form = variant.split("/")
    name, *flags = form.split("+")
    jit = kernel.startswith("jit_stage")
    jflags = kernel[kernel.find("[") + 1:-1].split(",") if jit else []
    if ("carry" in flags or "carry_only" in flags) and name not in ("feedback", "replay"):
        return "+carry on a launch that does not stride" if name != "strided" else "+carry on strided (no feedback)"
    if "defer" in jflags and (not feedback or carry_only is False):
        return "defer without carry_only"
    if name in ("feedback", "replay") and carry_only is not None and \
            ("carry_only" in flags, "carry" in flags) != (carry_only, not carry_only):
        return "a feedback launch whose carry flag is not the plan's"
    if "deep" in jflags and not feedback and block_option <= 1:
        return "deep in a plan without feedback unless FR_STAGE_BLOCK > 1"
    if name == "replay" and not feedback:
        return "replay without feedback"
    if feedback and name in ("fused", "strided", "levels"):
        return "fused / strided / levels in a feedback plan"
    return None
