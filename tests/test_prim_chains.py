"""Two-operation chains on the CPU (tests/prim_chains.py): the table is complete and its dropped rows are their twins' nodes; the
composed float64 expectation equals the C++ oracle and the numpy oracle on every chain, FOLD_SHAPES bodies included, in both
semantics; every chain runs through the engine's lowering, operand sort and planner on the host-logic simulator in pull and in
staged mode, where fr_plan_json must show that no chain was cut (the simulator's loops restate the kernels: this is NOT
arithmetic coverage of the engine -- tests/test_hip_prim_chains.py is); the voice recipes of the leaf chains and of FOLD_SHAPES
on the simulator (as stage programs: it has no run-time compiler); and, through tests/cpp/leaf_text.cpp, what the matcher and
leafjit.cpp make of every voice on the host: which chains a compiled voice takes (NOT_A_LEAF) and where the generated leaf holds
the fma fold and the abs idiom (the flags of FOLD_SHAPES)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import prim_chains as pc
import prim_pairs as pp
import sim_tools
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer
from test_proofs_sim import HOST_SOURCES, _graph_text, _host_program

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import ref_numpy  # noqa: E402

SEMANTICS = pp.SEMANTICS
FORM_LITERAL = [(form, L) for form in pc.FORMS for L in (pc.STAGE_LITERALS if pc.n_literals(form) else [None])]
FORM_LITERAL_IDS = [form if L is None else f"{form}-{L!r}" for form, L in FORM_LITERAL]
literal_sets_of = pc.literal_sets_of


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def test_the_table_is_complete():
    """Every (O, I) pair in every form, each side: a row of the table or the stated twin of one."""
    for form in pc.FORMS:
        rows = set(pc.ROWS[form])
        assert len(rows) == len(pc.ROWS[form]) <= 50
        for O in pc.OPS:
            for I in pc.OPS:
                for side in (0, 1):
                    tO, tI, tside, tform = pc.twin(O, I, side, form)
                    assert (tO, tI) == (O, I) and (tO, tI, tside) in pc.ROWS[tform], (O, I, side, form)
                    assert pc.twin(tO, tI, tside, tform) == (tO, tI, tside, tform)
                    if (O, I, side) not in rows:                       # dropped: only for a commutative op, and then never both sides / forms
                        assert (O in pc.COMMUTATIVE and side == 1) or (I in pc.COMMUTATIVE and form in ("LXY", "LXM")), (O, I, side, form)
    assert {f: len(r) for f, r in pc.ROWS.items()} == {"XYX": 40, "XYY": 40, "XLY": 40, "LXY": 24, "XYL": 40, "XLM": 40, "LXM": 24}
    assert [len(pc.literal_sets(f)) for f in pc.FORMS] == [1, 1, 8, 8, 8, 64, 64]
    assert len(pc.all_leaf_chains()) == 40 + 40 + 5 * (40 + 24 + 40) == 600
    assert sorted(np.array(pc.STAGE_LITERALS, np.float32).view(np.uint32).tolist()) == sorted(pp.STAGE_LITERALS.view(np.uint32).tolist())
    assert set(np.array(pc.LEAF_LITERALS, np.float32).view(np.uint32).tolist()) <= set(pp.STAGE_LITERALS.view(np.uint32).tolist())


def test_a_dropped_row_is_its_twins_node(sim):
    """Lowering gives a dropped chain the node of its twin: a graph of both rows lowers to as many nodes as the twin alone."""
    def lowered(exprs):
        with Renderer(sim, mode="pull") as r:
            synth.install(r, pc.rows_graph(exprs))
            r.fill_buffer(len(exprs), 0, 1, [np.zeros(1, np.float32)] * 2)
            return r.plan()["lowered_nodes"]
    dropped = 0
    for form in pc.FORMS:
        lits = (2.0, -0.5)[:pc.n_literals(form)]
        for O in pc.OPS:
            for I in pc.OPS:
                for side in (0, 1):
                    tO, tI, tside, tform = pc.twin(O, I, side, form)
                    if (tside, tform) == (side, form):
                        continue
                    dropped += 1
                    a, b = pc.chain_expr(O, I, side, form, lits), pc.chain_expr(tO, tI, tside, tform, lits)
                    assert pc.text(a) != pc.text(b) and lowered([b, a]) == lowered([b]), (pc.text(a), pc.text(b))
    assert dropped == 7 * 50 - sum(len(r) for r in pc.ROWS.values())


def test_the_inner_rounding_is_part_of_the_expectation():
    """Composing a chain in float64 WITHOUT rounding the inner result to f32 gives other bits: the expectation is the graph's
    two roundings, and the comparison with the oracles below would notice one rounding."""
    x, y = pp.both_blocks()
    with np.errstate(all="ignore"):
        once = (x.astype(np.float64) * y.astype(np.float64) + x.astype(np.float64)).astype(np.float32)
    twice = pc.evaluate(("Sum2", ("Multiply", "x", "y"), "x"), x, y)
    assert 100 < pp.differing(once, twice).sum() < len(x) // 2


# ---- the expectation against both oracles ----------------------------------------------------------------------------------------------
def check_against(render, form, L, what):
    inputs = pc.chain_inputs(form)
    for lits in literal_sets_of(form, L):
        exprs = [pc.chain_expr(O, I, side, form, lits) for O, I, side in pc.ROWS[form]]
        for semantics in SEMANTICS:
            got = render(pc.rows_graph(exprs), len(exprs), inputs, semantics)
            exp, A, B = pc.rows_expected(exprs, inputs, semantics)
            for r, e in enumerate(exprs):
                msg = pp.first_diff(pc.text(e), f"{form} {semantics} ({what})", A[r], B[r], got[r], exp[r])
                assert not msg, msg


def oracle_render(lib):
    def render(tree, n_rows, inputs, semantics):
        with Renderer(lib, semantics=semantics) as o:
            synth.install(o, tree)
            return o.fill_buffer(n_rows, 0, len(inputs[0]), inputs)
    return render


def numpy_render(tree, n_rows, inputs, semantics):
    with ref_numpy.NumpyRefRenderer(semantics=semantics) as o:
        synth.install(o, tree)
        return o.fill_buffer(n_rows, 0, len(inputs[0]), inputs)


@pytest.mark.parametrize("form,L", FORM_LITERAL, ids=FORM_LITERAL_IDS)
def test_expectation_equals_the_cpp_oracle(oracle_lib, form, L):
    check_against(oracle_render(oracle_lib), form, L, "C++ oracle")


@pytest.mark.parametrize("form,L", FORM_LITERAL, ids=FORM_LITERAL_IDS)
def test_expectation_equals_the_numpy_oracle(form, L):
    check_against(numpy_render, form, L, "numpy oracle")


def fold_exprs(kind):
    return [e for s in pc.FOLD_SHAPES if s["name"].startswith(kind) for e in s["exprs"]]


@pytest.mark.parametrize("kind", ["fma", "abs"])
def test_fold_shapes_equal_both_oracles(oracle_lib, kind):
    exprs = fold_exprs(kind)
    inputs = pc.fold_inputs(next(s for s in pc.FOLD_SHAPES if s["name"].startswith(kind)))
    for what, render in (("C++ oracle", oracle_render(oracle_lib)), ("numpy oracle", numpy_render)):
        for semantics in SEMANTICS:
            got = render(pc.rows_graph(exprs), len(exprs), inputs, semantics)
            exp, A, B = pc.rows_expected(exprs, inputs, semantics)
            for r, e in enumerate(exprs):
                msg = pp.first_diff(pc.text(e), f"FOLD_SHAPES {semantics} ({what})", A[r], B[r], got[r], exp[r])
                assert not msg, msg


# ---- every chain through the engine's host code: lowering, the operand sort, the planner --------------------------------------------------
@pytest.mark.parametrize("form,L", FORM_LITERAL, ids=FORM_LITERAL_IDS)
@pytest.mark.parametrize("ev", ["pull", "stage_kernel"])
def test_chains_on_the_simulator(sim, ev, form, L):
    """One renderer per (form, literal set, semantics); staged: a stage program per row, no ring, no copy program."""
    inputs = pc.chain_inputs(form)
    for lits in literal_sets_of(form, L):
        for semantics, rows in pc.stage_parts(form, ev):
            exprs = [pc.chain_expr(O, I, side, form, lits) for O, I, side in rows]
            got = pc.render_rows(sim, exprs, inputs, ev, semantics)
            exp, A, B = pc.rows_expected(exprs, inputs, semantics)
            for r, e in enumerate(exprs):
                msg = pp.first_diff(pc.text(e), f"{form} {semantics} on {ev} (simulator)", A[r], B[r], got[r], exp[r])
                assert not msg, msg


def test_a_duplicate_row_is_cut(sim):
    """What the no-cut assertion is for: with side 1 of a commutative outer op left in, two rows share a root and the plan gains
    a ring per shared root (10 for the 50 rows of XYX)."""
    exprs = [pc.chain_expr(O, I, side, "XYX") for O in pc.OPS for I in pc.OPS for side in (0, 1)]
    with Renderer(sim, mode="staged", options={"FR_STAGE_JIT": "0"}) as r:
        synth.install(r, pc.rows_graph(exprs))
        r.fill_buffer(len(exprs), 0, 1, [np.zeros(1, np.float32)] * 2)
        plan = r.plan()
    assert plan["rings"] == 10, (plan["rings"], plan["stage_programs"], plan["copy_programs"])
    with pytest.raises(AssertionError):
        pc.assert_no_cut(plan, len(exprs))


def test_stage_parts_fit_a_compiled_module():
    for form in pc.FORMS:
        for ev in pp.EVALUATORS:
            parts = pc.stage_parts(form, ev)
            for semantics in SEMANTICS:
                rows = [r for s, part in parts if s == semantics for r in part]
                assert rows == pc.stage_rows(form, semantics)                          # every row, once, in order
            assert all(len(part) <= (pc.STAGE_JIT_MAX_SHAPES if ev == "stage_jit" else 50) for _, part in parts)
        assert pc.stage_rows(form, "reference") == list(pc.ROWS[form])
        assert all(pc.holds_minimum(pc.chain_expr(*r, form, (1.0, 1.0)[:pc.n_literals(form)])) == (r in pc.stage_rows(form, "sparkle")) for r in pc.ROWS[form])


# ---- the voice recipes on the simulator (stage programs there) --------------------------------------------------------------------------
LEAF_FORM_LITERAL = [(form, lits[0] if lits else None) for form in pc.LEAF_FORMS for lits in pc.literal_sets(form, pc.LEAF_LITERALS)]
LEAF_FORM_LITERAL_IDS = [form if L is None else f"{form}-{L!r}" for form, L in LEAF_FORM_LITERAL]


@pytest.mark.parametrize("form,L", LEAF_FORM_LITERAL, ids=LEAF_FORM_LITERAL_IDS)
def test_leaf_chain_recipes_on_the_simulator(sim, form, L):
    """The voices of a leaf form (P = 32 leaves 2^-(k + 1) * chain) against the expectation through tree_sum: the recipe's scales
    and association, on H and 512 random patterns in x with y reversed."""
    x = pp.signal_row()
    inputs = [x, x[::-1].copy()]
    exprs = pc.leaf_chains(form, () if L is None else (L,))
    for semantics in SEMANTICS:
        sel = [e for e in exprs if semantics in pc.semantics_of(e)]
        got = pp.render_leaves(sim, pc.voices_graph(sel), len(sel), inputs, pc.LEAF_P, 1, semantics=semantics, compiled=False)
        exp, A, B = pc.voices_expected(sel, inputs, semantics)
        for r, e in enumerate(sel):
            msg = pp.first_diff(pc.text(e), f"leaves {form} {semantics} (simulator)", A[r], B[r], got[r], exp[r])
            assert not msg, msg


@pytest.mark.parametrize("kind", ["fma", "abs"])
def test_fold_shape_recipes_on_the_simulator(sim, kind):
    x = pp.signal_row()
    inputs = [x, x[::-1].copy()] if kind == "fma" else [x]
    for shape in pc.FOLD_SHAPES:
        if not shape["name"].startswith(kind):
            continue
        for semantics in sorted({s for _, s in pc.fold_settings(shape)}):
            for e in shape["exprs"]:                          # (a renderer each: the operand orders of one shape lower to one root)
                got = pp.render_leaves(sim, pc.voices_graph([e]), 1, inputs, pc.LEAF_P, 1, semantics=semantics, compiled=False)
                exp, A, B = pc.voices_expected([e], inputs, semantics)
                msg = pp.first_diff(pc.text(e), f"FOLD_SHAPES {semantics} (simulator)", A[0], B[0], got[0], exp[0])
                assert not msg, msg


# ---- the matcher and leafjit.cpp on the host: which chains a compiled voice takes, and what its leaf holds ----------------------------------
def leaf_texts(items):
    """[(exprs, semantics, fma)] -> per item, per voice, the dict tests/cpp/leaf_text.cpp prints."""
    text = "\n".join(_graph_text(pc.voices_graph(exprs), s == "sparkle", len(exprs)).replace("\n", f" {int(fma == '1')}\n", 1) for exprs, s, fma in items)
    p = subprocess.run([_host_program("leaf_text", HOST_SOURCES, "-O1")], input=text + "\n", capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = [json.loads(l) for l in p.stdout.splitlines()]
    assert len(out) == sum(len(exprs) for exprs, _, _ in items)
    it = iter(out)
    return [[next(it) for _ in exprs] for exprs, _, _ in items]


def test_not_a_leaf_is_within_its_cap():
    leaf = {pc.text(e) for e in pc.all_leaf_chains()}
    assert len(leaf) == 600 and set(pc.NOT_A_LEAF) <= leaf and 10 * len(pc.NOT_A_LEAF) <= len(leaf)
    assert not set(pc.NOT_A_LEAF) & {pc.text(e) for s in pc.FOLD_SHAPES for e in s["exprs"]}
    assert all(isinstance(rule, str) and rule for rule in pc.NOT_A_LEAF.values())


def test_the_matcher_takes_every_leaf_chain_but_the_listed():
    """match.cpp on the host (the device's plan is what tests/test_hip_prim_chains.py asserts): every leaf chain is a voice of 32
    leaves whose one varying parameter is the scale, except the chains of NOT_A_LEAF, which are none."""
    exprs = pc.all_leaf_chains()
    for e, voice in zip(exprs, leaf_texts([(exprs, "reference", "1")])[0]):
        assert voice["jit"] == (pc.text(e) not in pc.NOT_A_LEAF), pc.text(e)
        if voice["jit"]:
            assert voice["k"] == 1 and voice["log2_p"] == 5, (pc.text(e), voice["k"], voice["log2_p"])


def test_fold_shapes_hold_their_folds_in_the_generated_leaf():
    """leafjit.cpp's text for every voice of FOLD_SHAPES under every setting: __builtin_fmaf( and -__builtin_fabsf( exactly where
    the table's flags say (the same check reads the device's FR_JIT_DUMP in tests/test_hip_prim_chains.py)."""
    items = [(shape, fma, s, e) for shape in pc.FOLD_SHAPES for fma, s in pc.fold_settings(shape) for e in shape["exprs"]]
    voices = leaf_texts([([e], s, fma) for _, fma, s, e in items])
    for (shape, fma, s, e), (voice,) in zip(items, voices):
        assert voice["jit"] and voice["k"] == 1 and voice["log2_p"] == 5, (shape["name"], pc.text(e))
        pc.check_fold_source(shape, fma, voice["text"])
    assert sum(s["fma"] for s in pc.FOLD_SHAPES) == 12 and sum(s["abs"] for s in pc.FOLD_SHAPES) == 2
    # prim_pairs' "FMA" form has an input under the product, whose bound is infinite: no fold under either setting
    control = leaf_texts([([("Sum2", "x", ("Multiply", float(c), "y")) for c in pp.FMA_LITERALS], "reference", fma) for fma in ("1", "0")])
    assert all(v["jit"] and pc.FMA_MARK not in v["text"] for vs in control for v in vs)
