"""Two-operation chains (tests/prim_chains.py) on the device: every chain of the table on pull_kernel, stage_kernel and the
hipRTC-compiled stage programs, every leaf chain and every FOLD_SHAPES body as a hipRTC-compiled voice, against the composed
float64 expectation, bit for bit, every sample compared.  Each test asserts from fr_plan_json that the evaluator it names ran,
the staged ones also that no chain was cut (a stage program per row, no ring, no copy program).

Generated code is read back through FR_JIT_DUMP (every renderer has a hipRTC cache of its own, so each renderer's sources are
dumped): a compiled stage module must spell every literal of its graph as f32(0x...u) -- baked, not a parameter -- and hold
jit_mod1( exactly where a Modulo divides by the literal 1; a FOLD_SHAPES voice must hold __builtin_fmaf( and -__builtin_fabsf(
exactly where the table's flags say.

A compiled stage module holds at most 32 shapes and every row of a form is one, so the 40 rows of a form are two renderers of
20 on stage_jit (prim_chains.stage_parts); the parts of a form are tests of their own."""
import sys

import numpy as np
import pytest

import prim_chains as pc
import prim_pairs as pp

pytestmark = pytest.mark.gpu

SEMANTICS = pp.SEMANTICS


def spelled(L):
    return f"f32({int(np.float32(L).view(np.uint32)):#010x}u)"


@pytest.fixture(scope="module")
def compiled():
    """Counts for profiles/prim_chains.txt: hipRTC kernels compiled by this file's renderers."""
    counts = {"stage modules": [], "voices": []}
    yield counts
    print(f"\nprim_chains: jit_kernels_compiled: {sum(counts['stage modules'])} stage modules in {len(counts['stage modules'])} renderers, "
          f"{sum(counts['voices'])} voice kernels", file=sys.stderr)


# ---- the stage evaluators ----------------------------------------------------------------------------------------------------------
STAGE_CASES = [(ev, form, L, part) for ev in pp.EVALUATORS for form in pc.FORMS for L in (pc.STAGE_LITERALS if pc.n_literals(form) else [None])
               for part in range(len(pc.stage_parts(form, ev)))]


@pytest.mark.parametrize("ev,form,L,part", STAGE_CASES, ids=[f"{ev}-{form}" + ("" if L is None else f"-{L!r}") + f"-{part}" for ev, form, L, part in STAGE_CASES])
def test_chains_on_the_stage_evaluators(hip_lib, compiled, ev, form, L, part, tmp_path, monkeypatch):
    """One renderer per literal set: (), (L,), or (L, M) for the eight M.  Its rows are the part's rows of the form, every
    constant of the graph a literal of the set."""
    semantics, rows = pc.stage_parts(form, ev)[part]
    inputs = pc.chain_inputs(form)
    for n, lits in enumerate(pc.literal_sets_of(form, L)):
        exprs = [pc.chain_expr(O, I, side, form, lits) for O, I, side in rows]
        dump = tmp_path / str(n)
        if ev == "stage_jit":
            dump.mkdir()
            monkeypatch.setenv("FR_JIT_DUMP", str(dump))
        counts = []
        got = pc.render_rows(hip_lib, exprs, inputs, ev, semantics, counts)
        if ev == "stage_jit":
            compiled["stage modules"] += counts
            dumped = sorted(dump.glob("jit_stage_*.hip"))
            assert len(dumped) == 1 and counts == [1], f"expected one generated stage source of this renderer, found {len(dumped)} (compiled: {counts})"
            source = dumped[0].read_text()
            assert all(spelled(v) in source for v in lits) and "f32(P[" not in source, (lits, "a constant was not baked")
            assert ("jit_mod1(v" in source) == pc.has_mod1(exprs), lits
        exp, A, B = pc.rows_expected(exprs, inputs, semantics)
        for r, e in enumerate(exprs):
            msg = pp.first_diff(pc.text(e), f"{form} {semantics} on {ev}", A[r], B[r], got[r], exp[r])
            assert not msg, msg


# ---- compiled voice leaves (leafjit.cpp: jit_bank) --------------------------------------------------------------------------------------
LEAF_CASES = [(form, L, O) for form in pc.LEAF_FORMS for L in (pc.LEAF_LITERALS if pc.n_literals(form) else [None]) for O in pc.OPS]


@pytest.mark.parametrize("form,L,O", LEAF_CASES, ids=[form + ("" if L is None else f"-{L!r}") + f"-{O}" for form, L, O in LEAF_CASES])
def test_chains_in_compiled_voices(hip_lib, compiled, form, L, O):
    """The voices of one outer op (5 inner ops, both sides unless O commutes), one renderer per semantics: each voice a
    hipRTC-compiled bank of 32 leaves whose one varying parameter is the scale -- or, listed in NOT_A_LEAF, no bank at all."""
    inputs = pc.chain_inputs(form)
    exprs = pc.leaf_chains(form, () if L is None else (L,), O)
    assert len(exprs) == (3 if form == "LXY" else 5) * (1 if O in pc.COMMUTATIVE else 2)      # (LXY: the three inner ops that do not commute)
    for semantics in SEMANTICS:
        sel = [e for e in exprs if semantics in pc.semantics_of(e)]
        got = pc.render_voices(hip_lib, sel, inputs, semantics)
        compiled["voices"].append(sum(pc.text(e) not in pc.NOT_A_LEAF for e in sel))
        exp, A, B = pc.voices_expected(sel, inputs, semantics)
        for r, e in enumerate(sel):
            msg = pp.first_diff(pc.text(e), f"leaves {form} {semantics}", A[r], B[r], got[r], exp[r])
            assert not msg, msg


@pytest.mark.parametrize("shape", pc.FOLD_SHAPES, ids=[s["name"].replace(" ", "_") for s in pc.FOLD_SHAPES])
def test_fold_shapes_in_compiled_voices(hip_lib, compiled, shape, tmp_path, monkeypatch):
    """Every operand order of the shape is a voice in a renderer of its own (the orders lower to one root), under every setting
    of the shape: the dumped jit_bank source holds the folds exactly where the table's flags say, and the rows are the
    expectation's."""
    inputs = pc.fold_inputs(shape)
    for fma, semantics in pc.fold_settings(shape):
        for n, e in enumerate(shape["exprs"]):
            dump = tmp_path / f"{fma}_{semantics}_{n}"
            dump.mkdir()
            monkeypatch.setenv("FR_JIT_DUMP", str(dump))
            assert pc.text(e) not in pc.NOT_A_LEAF
            got = pc.render_voices(hip_lib, [e], inputs, semantics, options={"FR_JIT_FMA": fma})
            compiled["voices"].append(1)
            dumped = sorted(dump.glob("jit_bank_*.hip"))
            assert len(dumped) == 1, f"expected one generated voice source of this renderer, found {len(dumped)}"
            pc.check_fold_source(shape, fma, dumped[0].read_text())
            exp, A, B = pc.voices_expected([e], inputs, semantics)
            msg = pp.first_diff(pc.text(e), f"FOLD_SHAPES {shape['name']} FR_JIT_FMA={fma} {semantics}", A[0], B[0], got[0], exp[0])
            assert not msg, msg
