"""Two-operation chains of the five arithmetic primitives: the table, the graphs that carry a chain to each evaluator, and the
expectation composed from prim_pairs.reference (plain data and graph recipes: importable without a GPU).  tests/prim_pairs.py is
systematic for ONE operation; every fold a compiler applies needs two operations in reach of each other, often beside a baked
literal (a negate folded into its consumer, a select turned into v_min_f32, 0 - y, a multiply contracted into its add,
min(min(x, c), d)).  tests/test_prim_chains.py pins the expectation to both oracles and runs every chain through the engine's host
code on the simulator; tests/test_hip_prim_chains.py runs every chain on the device.

Chains.  A chain is (O, I, side, form, literals): the outer op O takes the inner op I as its left (side 0) or right (side 1)
operand.  x = In0, y = In1, L and M constants shared by the whole graph (baked literals of generated code).  Side 0:

    XYX  O(I(x, y), x)      XYY  O(I(x, y), y)      a value meets itself one level up              both_blocks(), 6305 frames
    XLY  O(I(x, L), y)      LXY  O(I(L, x), y)      XYL  O(I(x, y), L)                               both_blocks()
    XLM  O(I(x, L), M)      LXM  O(I(L, x), M)                                                      signal_row(), 559 frames

Expressions are nested tuples (op, a, b) over "x", "y" and float constants; `evaluate` composes prim_pairs.reference bottom up,
so every intermediate result is rounded to f32 as the graph rounds it: reference(O, reference(I, p, q, s), r, s).  Both semantics
where the chain holds a Minimum, the reference's alone elsewhere.  Every sample is compared, NaN equal to NaN, +0 different from -0."""
import numpy as np

import prim_pairs as pp
from libfriendship_amd import synth

OPS, KIND, SEMANTICS = pp.OPS, pp.KIND, pp.SEMANTICS
COMMUTATIVE = ("Sum2", "Multiply")
BODY = {"XYX": "xyx", "XYY": "xyy", "XLY": "xLy", "LXY": "Lxy", "XYL": "xyL", "XLM": "xLM", "LXM": "LxM"}   # inner a, inner b, the outer's other operand
FORMS = tuple(BODY)
STAGE_LITERALS = [float(v) for v in pp.STAGE_LITERALS]


# ---- expressions -------------------------------------------------------------------------------------------------------------
def text(e):
    """Sum2(Modulo(x, -0.0), y): an expression's spelling (the key of NOT_A_LEAF, the id of a test)."""
    return e if isinstance(e, str) else f"{e[0]}({text(e[1])}, {text(e[2])})" if isinstance(e, tuple) else repr(float(e))


def holds_minimum(e):
    return isinstance(e, tuple) and (e[0] == "Minimum" or holds_minimum(e[1]) or holds_minimum(e[2]))


def semantics_of(e):
    return SEMANTICS if holds_minimum(e) else SEMANTICS[:1]


def evaluate(e, x, y=None, semantics="reference"):
    """The f32 row of an expression: prim_pairs.reference per operation, each result rounded to f32 before the next uses it."""
    if isinstance(e, str):
        return {"x": x, "y": y}[e]
    if isinstance(e, tuple):
        return pp.reference(e[0], evaluate(e[1], x, y, semantics), evaluate(e[2], x, y, semantics), semantics)
    return np.float32(e)


def outer_operands(e, x, y=None, semantics="reference"):
    """The two operands of the expression's last operation, for prim_pairs.first_diff."""
    return evaluate(e[1], x, y, semantics), evaluate(e[2], x, y, semantics)


def _operand(g, e, n):
    if isinstance(e, str):
        return synth.IN("xy".index(e))
    if isinstance(e, tuple):
        return g.binop(KIND[e[0]], _operand(g, e[1], n), _operand(g, e[2], n), n)
    return synth.C(np.float32(e))


def rows_graph(exprs):
    """An output row per expression (the stage evaluators' graphs).  Equal sub-expressions of different rows are written again;
    lowering interns them."""
    g = synth.GraphArrays()
    return pp._rows(g, np.concatenate([_operand(g, e, 1) for e in exprs]))


def rows_expected(exprs, inputs, semantics):
    """[len(exprs), T] and the operands (A, B) of every row's last operation."""
    exp = np.stack([evaluate(e, *inputs, semantics=semantics) for e in exprs])
    ab = [outer_operands(e, *inputs, semantics=semantics) for e in exprs]
    return exp, np.stack([np.broadcast_to(a, exp.shape[1:]) for a, _ in ab]), np.stack([np.broadcast_to(b, exp.shape[1:]) for _, b in ab])


# ---- the table -----------------------------------------------------------------------------------------------------------------
def twin(O, I, side, form):
    """The chain whose lowered node this one shares -- itself for a row of the table.  Lowering sorts the operands of Sum2 and
    Multiply by node id (graph.cpp FlatGraph::make), so side 1 of a commutative outer op is side 0's node, and I(L, x) of a
    commutative inner op is I(x, L)'s: LXY is XLY's node, LXM is XLM's.  Such rows are dropped: two rows of one graph that share a
    root make the planner cut that root out into a ring (10 rings for the 50 rows of XYX), which is not what is under test."""
    if O in COMMUTATIVE:
        side = 0
    if I in COMMUTATIVE:
        form = {"LXY": "XLY", "LXM": "XLM"}.get(form, form)
    return O, I, side, form


ROWS = {form: tuple((O, I, side) for O in OPS for I in OPS for side in (0, 1) if twin(O, I, side, form) == (O, I, side, form)) for form in FORMS}


def n_literals(form):
    return sum(BODY[form].count(c) for c in "LM")


def two_signals(form):
    return "y" in BODY[form]


def literal_sets(form, literals=STAGE_LITERALS):
    """What L (and M) run over: (), (L,) for each literal, (L, M) for all pairs."""
    return [()] if n_literals(form) == 0 else [(L,) for L in literals] if n_literals(form) == 1 else [(L, M) for L in literals for M in literals]


def literal_sets_of(form, L, literals=STAGE_LITERALS):
    """The literal sets of one test (form, L): (), (L,), or (L, M) for every M.  (Compared by spelling: -0.0 == 0.0.)"""
    return [lits for lits in literal_sets(form, literals) if not lits or repr(lits[0]) == repr(L)]


def chain_expr(O, I, side, form, literals=()):
    tok = dict(zip("LM", literals), x="x", y="y")
    a, b, c = (tok[k] for k in BODY[form])
    return (O, (I, a, b), c) if side == 0 else (O, c, (I, a, b))


def chain_inputs(form):
    """The input rows of a form: both blocks (x, y), or the signal row (x)."""
    return list(pp.both_blocks()) if two_signals(form) else [pp.signal_row()]


def stage_rows(form, semantics):
    """The rows of a form's renderer under `semantics`: every row of the table under the reference's, the rows that hold a Minimum
    under Sparkle's (the others compute the same there)."""
    return [r for r in ROWS[form] if semantics == "reference" or "Minimum" in r[:2]]


# A compiled stage module holds at most 32 shapes (engine.cpp's call of plan_stage_jit), and every row here is a shape of its own:
# the 40 rows of a form run as two renderers of 20 on the hipRTC-compiled evaluator.  One constant per graph either way.
STAGE_JIT_MAX_SHAPES = 32


def stage_parts(form, ev):
    """[(semantics, rows)]: the renderers that carry a form (for one literal set) on evaluator `ev`."""
    parts = []
    for semantics in SEMANTICS:
        rows = stage_rows(form, semantics)
        if ev == "stage_jit" and len(rows) > STAGE_JIT_MAX_SHAPES:
            parts += [(semantics, rows[:len(rows) // 2]), (semantics, rows[len(rows) // 2:])]
        else:
            parts.append((semantics, rows))
    return parts


def assert_no_cut(plan, n_rows):
    """A staged plan of chains: a stage program per row, nothing cut out of a chain into a ring, no copy program."""
    assert plan["stage_programs"] == n_rows and plan["rings"] == 0 and plan["copy_programs"] == 0, (plan["stage_programs"], n_rows, plan["rings"], plan["copy_programs"])


def render_rows(lib, exprs, inputs, ev, semantics, compiled=None):
    """prim_pairs.render (which asserts the evaluator from the plan), with the no-cut assertions for the staged ones.
    compiled: a list that gets the plan's jit_kernels_compiled."""
    def check(plan):
        if ev != "pull":
            assert_no_cut(plan, len(exprs))
        if compiled is not None:
            compiled.append(plan["jit_kernels_compiled"])
    return pp.render(lib, rows_graph(exprs), len(exprs), inputs, ev, semantics, check_plan=check)


def has_mod1(exprs):
    """Does some Modulo of these expressions divide by the literal +1 (generated code: jit_mod1)?"""
    def walk(e):
        return isinstance(e, tuple) and ((e[0] == "Modulo" and not isinstance(e[2], (str, tuple)) and np.float32(e[2]).view(np.uint32) == 0x3F800000)
                                         or walk(e[1]) or walk(e[2]))
    return any(walk(e) for e in exprs)


# ---- compiled voice leaves: a voice of P leaves 2^-(k + 1) * body, as prim_pairs.leaf_graph --------------------------------------
LEAF_P = 32
LEAF_FORMS = ("XYX", "XYY", "XLY", "LXY", "XYL")      # (no two-literal forms: each voice is one hipRTC compile)
# the literals leafjit.cpp treats specially: opaque zeros, jit_mod1 / fract, the -1 of the abs idiom, a power of two
LEAF_LITERALS = [0.0, -0.0, 1.0, -1.0, 2.0]


def leaf_chains(form, literals=(), O=None):
    """The expressions of a leaf form with one literal set (and one outer op)."""
    return [chain_expr(o, I, side, form, literals) for o, I, side in ROWS[form] if O is None or o == O]


def all_leaf_chains():
    return [e for form in LEAF_FORMS for lits in literal_sets(form, LEAF_LITERALS) for e in leaf_chains(form, lits)]


def voices_graph(exprs, P=LEAF_P):
    """A voice (an output row) per expression: the balanced sum of P leaves 2^-(k + 1) * expression."""
    g = synth.GraphArrays()
    roots = [synth.sum_tree(g, g.binop(synth.K_MUL, synth.C(pp.leaf_scales(P)), _operand(g, e, P), P).reshape(1, P)) for e in exprs]
    return pp._rows(g, np.concatenate(roots))


def voices_expected(exprs, inputs, semantics, P=LEAF_P):
    """[len(exprs), T] through prim_pairs.tree_sum, and the operands (A, B) of every body's last operation."""
    exp, A, B = rows_expected(exprs, inputs, semantics)
    return pp.tree_sum(pp.reference("Multiply", pp.leaf_scales(P)[None, None, :], exp[..., None])), A, B


# Chains that the matcher (match.cpp match_shape_voice) refuses as a compiled voice, by spelling (`text`), with the rule that
# refuses them.  They run as stage programs and are compared all the same.  Asserted to be exact on the device: a listed chain
# that does compile fails tests/test_hip_prim_chains.py.  At most a tenth of the leaf chains, and no FOLD_SHAPES entry.
NOT_A_LEAF = {}


def render_voices(lib, exprs, inputs, semantics, options=None, P=LEAF_P):
    """The voices of `exprs` in mode "auto": those not in NOT_A_LEAF through prim_pairs.render_leaves (every one a hipRTC-compiled
    bank of P leaves whose one varying parameter is the scale), the listed ones in a renderer of their own whose plan must hold
    no bank.  Returns the rows in the order of `exprs`."""
    from libfriendship_amd.capi import Renderer
    leaf = [i for i, e in enumerate(exprs) if text(e) not in NOT_A_LEAF]
    other = [i for i, e in enumerate(exprs) if text(e) in NOT_A_LEAF]
    got = np.empty((len(exprs), len(inputs[0])), np.float32)
    if leaf:
        got[leaf] = pp.render_leaves(lib, voices_graph([exprs[i] for i in leaf], P), len(leaf), inputs, P, 1, options=options, semantics=semantics)
    if other:
        with Renderer(lib, options=options, semantics=semantics) as r:
            synth.install(r, voices_graph([exprs[i] for i in other], P))
            got[other] = r.fill_buffer(len(other), 0, len(inputs[0]), inputs)
            plan = r.plan()
        assert plan["pull_rows"] == 0 and not plan["banks"], ("listed in NOT_A_LEAF, but compiled as a voice", [text(exprs[i]) for i in other], plan["banks"])
    return got


# ---- FOLD_SHAPES: deeper bodies that reach leafjit.cpp's own folds ------------------------------------------------------------------
# fma: Sum2(y, Multiply(C(c), Modulo(x, C(d)))).  leafjit.cpp contracts y + c * v into one fma when c is a literal +-2^k, k >= 1,
# and |c| * bound[v] <= 1e38 (the product is exact and finite: one rounding either way).  bound[Modulo(., d)] = 2 |d|, so c in
# {+-2, +-4} with d in {1, 0.75, 3} must fold under FR_JIT_FMA=1; c = 2^126 with d = 3 gives 2 * 3 * 2^126 > 1e38 and must not.
# (An input's bound is infinite: Sum2(In0, Multiply(C(c), In1)), prim_pairs' "FMA" form, never folds.)  x, y: both_blocks().
# abs idiom: Minimum(v, Multiply(C(-1), v)) is -|v| bit for bit unless v is -0 (the graph gives +0 there), so it becomes
# -__builtin_fabsf(v) where v can be proven never -0: v = Sum2(C(1), x) and Sum2(C(+0), x) (a sum is -0 only if both terms are),
# not v = x, Sum2(C(-0), x), Minimum(C(1), x).  The mirror Minimum(Multiply(C(-1), v), v) is +0 at v = +0 where -|v| is -0: it
# must never fold.  x: signal_row(), both semantics.
FMA_C = [2.0, -2.0, 4.0, -4.0]
FMA_D = [1.0, 0.75, 3.0]
FMA_TOO_LARGE = (2.0 ** 126, 3.0)
FMA_MARK, ABS_MARK = "__builtin_fmaf(", "-__builtin_fabsf("


def _fma_orders(c, d):
    m = ("Modulo", "x", d)
    return [("Sum2", "y", ("Multiply", c, m)), ("Sum2", ("Multiply", c, m), "y"), ("Sum2", "y", ("Multiply", m, c)), ("Sum2", ("Multiply", m, c), "y")]


ABS_V = [("x", False), (("Sum2", -0.0, "x"), False), (("Minimum", 1.0, "x"), False), (("Sum2", 1.0, "x"), True), (("Sum2", 0.0, "x"), True)]   # (v, never -0)

# {"name", "exprs" (operand orders of one shape: each a voice), "fma" / "abs": must the generated source hold the fold}
FOLD_SHAPES = [{"name": f"fma c={c!r} d={d!r}", "exprs": _fma_orders(c, d), "fma": True, "abs": False} for c in FMA_C for d in FMA_D]
FOLD_SHAPES.append({"name": "fma c=2^126 d=3.0", "exprs": _fma_orders(*FMA_TOO_LARGE), "fma": False, "abs": False})
FOLD_SHAPES += [{"name": f"abs v={text(v)}", "exprs": [("Minimum", v, ("Multiply", -1.0, v))], "fma": False, "abs": never_negzero} for v, never_negzero in ABS_V]
FOLD_SHAPES += [{"name": f"abs mirror v={text(v)}", "exprs": [("Minimum", ("Multiply", -1.0, v), v)], "fma": False, "abs": False} for v, _ in ABS_V]


def fold_inputs(shape):
    return list(pp.both_blocks()) if shape["name"].startswith("fma") else [pp.signal_row()]


def fold_settings(shape):
    """[(FR_JIT_FMA, semantics)] a shape runs under: the fma shapes with the fold on and off, the abs idiom in both semantics."""
    return [("1", "reference"), ("0", "reference")] if shape["name"].startswith("fma") else [("1", s) for s in SEMANTICS]


def check_fold_source(shape, fma, source):
    """The generated source of one voice of a FOLD_SHAPES entry holds each fold exactly where the table's flag says."""
    want_fma, want_abs = shape["fma"] and fma == "1", shape["abs"]
    assert (FMA_MARK in source) == want_fma, (shape["name"], f"FR_JIT_FMA={fma}", "__builtin_fmaf( " + ("missing" if want_fma else "present"))
    assert (ABS_MARK in source) == want_abs, (shape["name"], "-__builtin_fabsf( " + ("missing" if want_abs else "present"))
