"""The operand-pair matrix on the CPU (tests/prim_pairs.py): the float64 reference against the C++ oracle and the numpy
oracle on both blocks, all five ops, both semantics; the both-constant form through the engine's own constant folder
(graph.cpp FlatGraph::make) in the host-logic simulator; the signal forms (SS, SP / PS, SL / LS) through the engine's lowering
and planning in the simulator, in pull and in staged mode, each asserted from fr_plan_json (the simulator's loops restate the
kernels: the HIP kernels themselves are not run here); the graphs that carry a pair to stage_tile_kernel, stage_sweep_kernel and a
streamed loop program, with the form each plan must take; and the comparison's own self-test."""
import os
import sys

import numpy as np
import pytest

import prim_pairs as pp
import sim_tools
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import ref_numpy  # noqa: E402

SEMANTICS = pp.SEMANTICS


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


def test_the_operand_set():
    bits = pp.H.view(np.uint32)
    assert len(pp.H) == 47 and np.isnan(pp.H).sum() == 1
    assert len(set(bits.tolist())) == 45            # 2^24 + 1 rounds to 2^24 as an f32: that magnitude is in the set twice
    assert 0x007FFFFF in bits and 0x00800000 in bits and 0x00000001 in bits and 0x80000000 in bits      # largest subnormal, FLT_MIN, 1e-45, -0
    assert 0x4B800000 in bits and 0x7F7FFFFF in bits and 0xFF800000 in bits                              # 2^24, FLT_MAX, -inf
    a, b = pp.pair_block()
    assert len(a) == len(b) == 2209 and {(x, y) for x, y in zip(a.view(np.uint32).tolist(), b.view(np.uint32).tolist())} == \
        {(x, y) for x in bits.tolist() for y in bits.tolist()}
    ra, rb = pp.random_block()
    assert len(ra) == len(rb) == 4096 and len(set(((ra.view(np.uint32) >> 23) & 0xFF).tolist())) == 256   # every exponent occurs


def test_the_pair_block_is_not_dominated_by_nan():
    a, b = pp.pair_block()
    for op in pp.OPS:
        r = pp.reference(op, a, b)
        assert np.isnan(r).mean() <= 0.125, op
        sub = (r != 0) & (np.abs(r) < np.float32(1.17549435e-38))
        assert sub.sum() >= 56, (op, int(sub.sum()))
        negzero = int((r.view(np.uint32) == 0x80000000).sum())
        assert negzero >= (1 if op == "Sum2" else 48), (op, negzero)


def test_the_comparison_tells_what_it_must():
    f = lambda bits: np.array([bits], np.uint32).view(np.float32)
    assert pp.differing(f(0x80000000), f(0x00000000)).all()                 # -0 against +0
    assert pp.differing(f(0x3F800001), f(0x3F800000)).all()                 # one ulp
    assert pp.differing(f(0x00000001), f(0x00000000)).all()                 # the smallest subnormal against zero
    assert not pp.differing(f(0x7FC00000), f(0xFFC00001)).any()             # NaN against NaN, any sign and payload
    assert pp.differing(f(0x7FC00000), f(0x7F800000)).all()                 # NaN against infinity
    assert not pp.differing(f(0x80000000), f(0x80000000)).any()
    msg = pp.first_diff("Divide", "SS", f(0x3F800000), f(0x40400000), f(0x3EAAAAAA), f(0x3EAAAAAB))
    assert "Divide SS" in msg and "0x3eaaaaaa" in msg and "0x3eaaaaab" in msg and "0x40400000" in msg and "1 of 1" in msg
    assert pp.first_diff("Sum2", "SS", f(0), f(0), f(0x7FC00000), f(0xFFC00000)) == ""


@pytest.fixture(scope="module")
def reference_rows():
    return pp.reference_rows()


@pytest.mark.parametrize("semantics", SEMANTICS)
def test_reference_equals_the_cpp_oracle(oracle_lib, reference_rows, semantics):
    a, b = pp.both_blocks()
    tree, meta = pp.ss_graph()
    with Renderer(oracle_lib, semantics=semantics) as o:
        synth.install(o, tree)
        got = o.fill_buffer(len(meta), 0, len(a), [a, b])
    for r, (op, form) in enumerate(meta):
        msg = pp.first_diff(op, f"{form} {semantics} (C++ oracle)", a, b, got[r], reference_rows[semantics][r])
        assert not msg, msg


@pytest.mark.parametrize("semantics", SEMANTICS)
def test_reference_equals_the_numpy_oracle(reference_rows, semantics):
    a, b = pp.both_blocks()
    tree, meta = pp.ss_graph()
    with ref_numpy.NumpyRefRenderer(semantics=semantics) as o:
        synth.install(o, tree)
        got = o.fill_buffer(len(meta), 0, len(a), [a, b])
    for r, (op, form) in enumerate(meta):
        msg = pp.first_diff(op, f"{form} {semantics} (numpy oracle)", a, b, got[r], reference_rows[semantics][r])
        assert not msg, msg


CC_FRAMES = pp.CC_FRAMES


def constant_rows(lib, op, semantics, mode="auto"):
    """op(C(a), C(b)) for the 2209 pairs of H x H, one node and one output row per pair, a call of CC_FRAMES frames: the rows
    (each must be constant over the call) and the plan."""
    a, b = pp.pair_block()
    with Renderer(lib, mode=mode, semantics=semantics) as r:
        synth.install(r, pp.cc_graph(op, a, b))
        got = r.fill_buffer(len(a), 0, CC_FRAMES, [np.zeros(CC_FRAMES, np.float32)])
        return got, r.plan()


def check_constant_rows(op, semantics, got, what):
    a, b = pp.pair_block()
    exp = pp.reference(op, a, b, semantics)
    msg = pp.first_diff(op, f"CC {semantics} ({what})", a[:, None], b[:, None], got, np.repeat(exp[:, None], CC_FRAMES, axis=1))
    assert not msg, msg


@pytest.mark.parametrize("semantics", SEMANTICS)
@pytest.mark.parametrize("op", pp.OPS)
def test_both_constant_form_through_the_constant_folder(sim, op, semantics):
    got, plan = constant_rows(sim, op, semantics)
    check_constant_rows(op, semantics, got, "simulator")
    # folded at lowering: what is left of 2209 binary nodes is constants (no input, no operation), one per distinct value.
    # (The plan has no count of operation nodes; the rows' values above are what proves the fold, this bound only that the
    # 2209 operations did not survive wholesale.)
    exp = pp.reference(op, *pp.pair_block(), semantics)
    distinct = len(set(np.where(np.isnan(exp), np.float32(np.nan), exp).view(np.uint32).tolist()))
    assert plan["lowered_nodes"] <= 2 * pp.N_H + distinct + 2, plan["lowered_nodes"]   # (+ 2: the sign and payload a NaN result may carry)


# ---- the signal forms through the engine's host code (lowering, CSE of mirrored rows, stage programs, plans) ------------------
EVALUATORS = ("pull", "stage_kernel")     # (the simulator has no run-time compiler: no "stage_jit")
render, semantics_of = pp.render, pp.semantics_of


@pytest.mark.parametrize("op", pp.OPS)
@pytest.mark.parametrize("ev", EVALUATORS)
def test_two_signals_on_the_simulator(sim, reference_rows, ev, op):
    """SS: op(In0, In1) on both blocks, 6305 frames."""
    a, b = pp.both_blocks()
    tree, _ = pp.ss_graph([op])
    for semantics in semantics_of(op):
        got = render(sim, tree, 1, [a, b], ev, semantics)
        msg = pp.first_diff(op, f"SS {semantics} on {ev}", a, b, got[0], reference_rows[semantics][pp.OPS.index(op)])
        assert not msg, msg


@pytest.mark.parametrize("op", pp.OPS)
@pytest.mark.parametrize("ev", EVALUATORS)
def test_signal_and_parameter_on_the_simulator(sim, ev, op):
    """SP / PS: op(In0, C(H[j])) and its mirror, a row per j (94 rows); the input is H and 512 random patterns."""
    x = pp.signal_row()
    tree, meta = pp.sp_graph([op])
    for semantics in semantics_of(op):
        got = render(sim, tree, len(meta), [x], ev, semantics)
        exp, A, B = pp.one_signal_expected(meta, x, semantics)
        msg = pp.first_diff(op, f"SP, PS {semantics} on {ev}", A, B, got, exp)
        assert not msg, msg


@pytest.mark.parametrize("semantics", SEMANTICS)
@pytest.mark.parametrize("literal", pp.STAGE_LITERALS, ids=[repr(float(v)) for v in pp.STAGE_LITERALS])
def test_signal_and_literal_on_the_simulator(sim, literal, semantics):
    """SL / LS: one renderer per literal, ten rows (five ops, two sides), every constant of the graph the same."""
    x = pp.signal_row()
    tree, meta = pp.sl_graph(literal)
    got = render(sim, tree, len(meta), [x], "stage_kernel", semantics)
    exp, A, B = pp.one_signal_expected(meta, x, semantics)
    for r, (op, form, _) in enumerate(meta):
        msg = pp.first_diff(op, f"{form} {literal!r} {semantics} on stage_kernel", A[r], B[r], got[r], exp[r])
        assert not msg, msg


# ---- the recipes of the generated leaves and of block streaming: their expectations and the serving rule, on the simulator -------
LEAF_P = 32      # the fewest leaves the matcher takes for a compiled voice (2^5 .. 2^13)


@pytest.mark.parametrize("op", pp.OPS)
def test_leaf_recipes_on_the_simulator(sim, op):
    """SS, SL / LS over the leaf literals, and the fma form: the simulator has no run-time compiler, so the voices run as stage
    programs; what this checks is the recipes' float64 expectation (scales, tree association)."""
    a, b = pp.both_blocks()
    x = pp.signal_row()
    for semantics in semantics_of(op):
        got = pp.render_leaves(sim, pp.leaf_graph(op, "SS", [0.0], LEAF_P), 1, [a, b], LEAF_P, 1, semantics=semantics, compiled=False)
        exp, A, B = pp.leaf_expected(op, "SS", [0.0], LEAF_P, a, b, semantics)
        msg = pp.first_diff(op, f"leaves SS {semantics}", A, B, got, exp)
        assert not msg, msg
        for form in ("SL", "LS"):
            got = pp.render_leaves(sim, pp.leaf_graph(op, form, pp.LEAF_LITERALS, LEAF_P), len(pp.LEAF_LITERALS), [x], LEAF_P, 1,
                                   semantics=semantics, compiled=False)
            exp, A, B = pp.leaf_expected(op, form, pp.LEAF_LITERALS, LEAF_P, x, None, semantics)
            msg = pp.first_diff(op, f"leaves {form} {semantics}", A, B, got, exp)
            assert not msg, msg
    if op == "Sum2":
        got = pp.render_leaves(sim, pp.leaf_graph(op, "FMA", pp.FMA_LITERALS, LEAF_P), 2, [a, b], LEAF_P, 1, compiled=False)
        exp, A, B = pp.leaf_expected(op, "FMA", pp.FMA_LITERALS, LEAF_P, a, b)
        msg = pp.first_diff(op, "leaves Sum2(x, Multiply(L, y))", A, B, got, exp)
        assert not msg, msg


@pytest.fixture(scope="module")
def stream_voices(oracle_lib):
    """The oracle's rendering of the six streaming voices on the time ramp of both blocks (used for the voice only)."""
    N = len(pp.both_blocks()[0])
    with Renderer(oracle_lib) as o:
        synth.install(o, pp.voices_tree(6, 128))
        v = o.fill_buffer(6, 0, N, [synth.time_ramp(0, N)])
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("bus", [False, True])
def test_stream_recipe_on_the_simulator(sim, stream_voices, bus):
    """Row v = Sum2(Multiply(voice_v, In1), op_v(In2, In3)) is servable with control rows (the Sum2 form, not the fallback),
    one program per voice or, summed in pairs, bus programs; through fr_fill_buffer the values equal the expectation."""
    import stream_input_cases as I
    a, b = pp.both_blocks()
    ops = pp.OPS + ("Minimum",) if bus else pp.OPS
    n = len(ops) // 2 if bus else len(ops)
    rows = [synth.time_ramp(0, len(a)), np.zeros(len(a), np.float32), a, b]
    with Renderer(sim, options=I.OPTION) as r:
        synth.install(r, pp.stream_graph(ops, bus=bus))
        got = r.fill_buffer(n, 0, len(a), rows)
        s = r.plan()["stream"]
    assert s["servable"] and s["input_slots"] == [0, 1, 2, 3] and s["bus_programs"] == (3 if bus else 0), s
    exp = pp.stream_expected(stream_voices[:len(ops)], rows[1], a, b, ops, bus=bus)
    msg = pp.first_diff("every op", f"stream bus={bus}", a, b, got, exp)
    assert not msg, msg


# ---- the interpreters of feedback plans and of streamed loop programs: the recipes, the forms and the expectations -------------------
@pytest.fixture(scope="module")
def loop_rows_expected():
    """{sweep: row 1 of loop_graph from the loop alone}, read-only."""
    out = {sweep: pp.loop_expected(sweep, pp.loop_rows(len(pp.both_blocks()[0]))) for sweep in (False, True)}
    for v in out.values():
        assert np.isfinite(v).all()
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("op", pp.OPS)
@pytest.mark.parametrize("sweep", [False, True], ids=["stage_tile_kernel", "stage_sweep_kernel"])
def test_two_signals_beside_a_loop_on_the_simulator(sim, reference_rows, loop_rows_expected, sweep, op):
    """op(In0, In1) on both blocks as a program of the tiled (the sweep) launch of a feedback plan whose loop it never meets:
    row 0 is the pair's reference, row 1 the loop's alone."""
    a, b = pp.both_blocks()
    for semantics in semantics_of(op):
        got = pp.render_beside_loop(sim, op, sweep, semantics)
        msg = pp.first_diff(op, f"SS {semantics} beside a loop, sweep={sweep}", a, b, got[0], reference_rows[semantics][pp.OPS.index(op)])
        assert not msg, msg
        msg = pp.first_diff("the loop", f"beside {op}, sweep={sweep}", 0, 0, got[1], loop_rows_expected[sweep])
        assert not msg, msg


@pytest.mark.parametrize("semantics", SEMANTICS)
def test_hostile_amounts_in_a_sweep_on_the_simulator(sim, semantics):
    """tests/loop_dyn_cases.py keeps every amount in [lo, hi] of its proof (its hostile call feeds the LFO, which clamps), so no
    case there has a negative, NaN, infinite, >= 2^64 or fractional amount: sweep_dyn_graph does, on every frame -- S_READ_DYN
    all of them but +inf and 2^64, which cannot reach a ring's read."""
    got, exp = pp.sweep_dyn_rows(sim, semantics)
    msg = pp.first_diff("Delay by a hostile amount", f"sweep {semantics}", 0, 0, got, exp)
    assert not msg, msg


def test_stream_loop_recipe_on_the_simulator(sim, reference_rows):
    """Row v = Sum2(Multiply(Multiply(x_v, x_v), In1), op_v(In2, In3)) with In1 a row of -0: served as ONE loop program per voice,
    and through fr_fill_buffer the rows are the pair's reference bit for bit -- the loop leaves no trace, not even on -0."""
    import stream_loop_cases as SL
    a, b = pp.both_blocks()
    for semantics in SEMANTICS:
        with Renderer(sim, options=SL.INPUTS, semantics=semantics) as r:
            synth.install(r, pp.stream_loop_graph())
            got = r.fill_buffer(len(pp.OPS), 0, len(a), pp.stream_loop_rows())
            pp.assert_loop_programs(r.plan()["stream"], len(pp.OPS))
        msg = pp.first_diff("every op", f"stream loop programs {semantics}", a, b, got, reference_rows[semantics])
        assert not msg, msg
