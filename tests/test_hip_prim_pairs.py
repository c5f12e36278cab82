"""The operand-pair matrix (tests/prim_pairs.py) on the device: op x operand form x evaluator against the float64 reference, bit
for bit, every sample compared.  Each test asserts from fr_plan_json that the evaluator it names is the one that ran.

Evaluators: pull_kernel (mode="pull": SS, SP / PS, CC), stage_kernel (mode="staged", FR_STAGE_JIT=0: SS, SP / PS, SL / LS), the
hipRTC-compiled stage programs (FR_STAGE_JIT=force: SS, SP / PS, SL / LS; for the literal forms the generated source is read back
through FR_JIT_DUMP to show that the constant was baked), the hipRTC-compiled voice leaves (SS, SL / LS, the fma form with
FR_JIT_FMA on and off -- a no-fold control: an input's product is never contracted; the fold is tests/test_hip_prim_chains.py's
FOLD_SHAPES --, Modulo(x, 1) in its fract and its general body), the three block-streaming interpreters, and the
interpreters that only a loop brings up: stage_tile_kernel and stage_sweep_kernel (SS beside a loop of a feedback plan, and the
Delays by a hostile amount in a sweep) and block streaming's loop programs (SS inside the loop's program).

What the leaf forms cannot carry as the design had it: a compiled voice has 32 to 8192 leaves (match.cpp), so P = 2 does not
exist, and P IDENTICAL leaves are one interned node; every leaf is the operation times its own power of two (prim_pairs.py).
A constant that is the same within a voice is a literal of that voice's kernel, so SP / PS (a constant as a PARAMETER of a
leaf) would need constants that differ within a voice, whose sum no longer shows one leaf's bits: not built."""
import numpy as np
import pytest

import prim_pairs as pp
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

pytestmark = pytest.mark.gpu

SEMANTICS, EVALUATORS, CC_FRAMES = pp.SEMANTICS, pp.EVALUATORS, pp.CC_FRAMES
render, semantics_of = pp.render, pp.semantics_of


@pytest.fixture(scope="module")
def reference_rows():
    return pp.reference_rows()


@pytest.mark.parametrize("op", pp.OPS)
@pytest.mark.parametrize("ev", list(EVALUATORS))
def test_two_signals(hip_lib, reference_rows, ev, op):
    """SS: op(In0, In1) on H x H and the 4096 random bit patterns, 6305 frames."""
    a, b = pp.both_blocks()
    tree, _ = pp.ss_graph([op])
    for semantics in semantics_of(op):
        got = render(hip_lib, tree, 1, [a, b], ev, semantics)
        msg = pp.first_diff(op, f"SS {semantics} on {ev}", a, b, got[0], reference_rows[semantics][pp.OPS.index(op)])
        assert not msg, msg


@pytest.mark.parametrize("op", pp.OPS)
@pytest.mark.parametrize("ev", list(EVALUATORS))
def test_signal_and_parameter(hip_lib, ev, op):
    """SP / PS: op(In0, C(H[j])) and its mirror, a row per j (94 rows): the constants differ from row to row, so generated code
    gets them as parameters.  The input is H and 512 random patterns."""
    x = pp.signal_row()
    tree, meta = pp.sp_graph([op])
    for semantics in semantics_of(op):
        got = render(hip_lib, tree, len(meta), [x], ev, semantics)
        exp, A, B = pp.one_signal_expected(meta, x, semantics)
        msg = pp.first_diff(op, f"SP, PS {semantics} on {ev}", A, B, got, exp)
        assert not msg, msg


@pytest.mark.parametrize("semantics", SEMANTICS)
@pytest.mark.parametrize("literal", pp.STAGE_LITERALS, ids=[repr(float(v)) for v in pp.STAGE_LITERALS])
@pytest.mark.parametrize("ev", ["stage_kernel", "stage_jit"])
def test_signal_and_literal(hip_lib, ev, literal, semantics, tmp_path, monkeypatch):
    """SL / LS: one renderer per literal, ten rows (five ops, two sides), every row a shape of its own and every constant of
    the graph the same, so a compiled stage program bakes it: the dumped source must hold the literal's f32(0x...u) spelling,
    and jit_mod1( exactly where the literal is +1 (Modulo(x, 1)).  The interpreter does not tell literals apart; it runs the
    same rows."""
    if ev == "stage_jit":
        monkeypatch.setenv("FR_JIT_DUMP", str(tmp_path))
    x = pp.signal_row()
    tree, meta = pp.sl_graph(literal)
    got = render(hip_lib, tree, len(meta), [x], ev, semantics)
    if ev == "stage_jit":
        dumped = sorted(tmp_path.glob("jit_stage_*.hip"))
        assert dumped, "no generated stage source was dumped: the programs of this case were compiled before, by another test"
        text = "".join(p.read_text() for p in dumped)
        assert f"f32({int(np.float32(literal).view(np.uint32)):#010x}u)" in text, literal
        assert ("jit_mod1(v" in text) == (np.float32(literal).view(np.uint32) == 0x3F800000), literal
        assert "jit_min(v" in text and "jit_mod(v" in text
    exp, A, B = pp.one_signal_expected(meta, x, semantics)
    for r, (op, form, _) in enumerate(meta):
        msg = pp.first_diff(op, f"{form} {literal!r} {semantics} on {ev}", A[r], B[r], got[r], exp[r])
        assert not msg, msg


@pytest.mark.parametrize("op", pp.OPS)
def test_both_constants_on_the_device_build(hip_lib, op):
    """CC: op(C(a), C(b)) for the 2209 pairs of H x H, a node and an output row per pair, folded by the device library's own
    build of the constant folder; what is left are constant rows for pull_kernel."""
    a, b = pp.pair_block()
    tree = pp.cc_graph(op, a, b)
    for semantics in semantics_of(op):
        with Renderer(hip_lib, mode="pull", semantics=semantics) as r:
            synth.install(r, tree)
            got = r.fill_buffer(len(a), 0, CC_FRAMES, [np.zeros(CC_FRAMES, np.float32)])
            plan = r.plan()
        assert plan["pull_rows"] == len(a) and not plan["stage_launches"] and not plan["banks"], plan["pull_rows"]
        exp = pp.reference(op, a, b, semantics)
        msg = pp.first_diff(op, f"CC {semantics} (device build)", a[:, None], b[:, None], got, np.repeat(exp[:, None], CC_FRAMES, axis=1))
        assert not msg, msg


# ---- generated voice leaves (leafjit.cpp: jit_bank) ------------------------------------------------------------------------------
@pytest.mark.parametrize("op,P", [(op, 32) for op in pp.OPS] + [("Divide", 64)])
def test_leaves_two_signals(hip_lib, op, P):
    """SS: one voice of P leaves 2^-(k + 1) * op(In0, In1) on both blocks; the one varying parameter is the scale."""
    a, b = pp.both_blocks()
    tree = pp.leaf_graph(op, "SS", [0.0], P)
    for semantics in semantics_of(op):
        got = pp.render_leaves(hip_lib, tree, 1, [a, b], P, 1, semantics=semantics)
        exp, A, B = pp.leaf_expected(op, "SS", [0.0], P, a, b, semantics)
        msg = pp.first_diff(op, f"leaves SS P={P} {semantics}", A, B, got, exp)
        assert not msg, msg


@pytest.mark.parametrize("form", ["SL", "LS"])
@pytest.mark.parametrize("op", pp.OPS)
def test_leaves_signal_and_literal(hip_lib, op, form):
    """SL / LS: a voice (and a kernel: 11 hipRTC compiles) per literal of {+-0, +-1, 0.5, 2, -2, 4, inf, NaN, 1e-45}; the
    constant is the same in every leaf, so it is baked and the scale stays the only parameter (leaf_params == 1).  The input
    is H and 512 random patterns; for Modulo(x, 1) see test_leaves_modulo_by_one_both_bodies."""
    x = pp.signal_row()
    tree = pp.leaf_graph(op, form, pp.LEAF_LITERALS, 32)
    for semantics in semantics_of(op):
        got = pp.render_leaves(hip_lib, tree, len(pp.LEAF_LITERALS), [x], 32, 1, semantics=semantics)
        exp, A, B = pp.leaf_expected(op, form, pp.LEAF_LITERALS, 32, x, None, semantics)
        msg = pp.first_diff(op, f"leaves {form} {semantics}", A, B, got, exp)
        assert not msg, msg


@pytest.mark.parametrize("fma", ["1", "0"])
def test_leaves_fma_fold(hip_lib, fma, tmp_path, monkeypatch):
    """Sum2(x, Multiply(L, y)) with L = 2 and -4 on both blocks, FR_JIT_FMA on and off.  This is the NO-FOLD control: leafjit.cpp
    contracts y + 2^k * v only where it can bound |2^k * v| <= 1e38, an input's bound is infinite, so both settings generate the
    same v + v code -- the dumped sources must hold no __builtin_fmaf( under either.  The fold itself is exercised by
    prim_chains.FOLD_SHAPES (tests/test_hip_prim_chains.py), whose products are bounded by a Modulo."""
    monkeypatch.setenv("FR_JIT_DUMP", str(tmp_path))
    a, b = pp.both_blocks()
    got = pp.render_leaves(hip_lib, pp.leaf_graph("Sum2", "FMA", pp.FMA_LITERALS, 32), 2, [a, b], 32, 1, options={"FR_JIT_FMA": fma})
    dumped = sorted(tmp_path.glob("jit_bank_*.hip"))
    assert len(dumped) == len(pp.FMA_LITERALS), f"expected a generated voice source per literal, found {len(dumped)}"
    assert not any("__builtin_fmaf(" in p.read_text() for p in dumped), "the control folds after all: an input's product was contracted"
    exp, A, B = pp.leaf_expected("Sum2", "FMA", pp.FMA_LITERALS, 32, a, b)
    msg = pp.first_diff("Sum2", f"leaves Sum2(x, Multiply(L, y)) FR_JIT_FMA={fma}", A, B, got, exp)
    assert not msg, msg


def test_leaves_modulo_by_one_both_bodies(hip_lib):
    """Modulo(x, 1): a call whose inputs all lie in [+0, 2^32] (the fract body where the host proved it exact) and a call with
    H and random patterns (the general body), same renderer."""
    inside = np.concatenate([pp.H[(pp.H.view(np.uint32) <= 0x4F800000)], np.abs(pp.random_block()[0][:512])])
    inside = inside[inside.view(np.uint32) <= 0x4F800000]
    assert len(inside) > 300 and 4294967296.0 in inside and 0.0 in inside
    tree = pp.leaf_graph("Modulo", "SL", [1.0], 32)
    for what, x in (("inputs in [+0, 2^32]", inside), ("hostile inputs", pp.signal_row())):
        got = pp.render_leaves(hip_lib, tree, 1, [x], 32, 1)
        exp, A, B = pp.leaf_expected("Modulo", "SL", [1.0], 32, x)
        msg = pp.first_diff("Modulo", f"leaves SL 1.0, {what}", A, B, got, exp)
        assert not msg, msg


# ---- the block-streaming interpreters --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stream_voices(oracle_lib):
    """The oracle's rendering of the six streaming voices on the time ramp of both blocks (used for the voice only)."""
    N = len(pp.both_blocks()[0])
    with Renderer(oracle_lib) as o:
        synth.install(o, pp.voices_tree(6, 128))
        v = o.fill_buffer(6, 0, N, [synth.time_ramp(0, N)])
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("bus", [False, True], ids=["voice_programs", "bus_programs"])
def test_stream_control_rows(hip_lib, stream_voices, bus):
    """bank_stream_in_kernel: row v = Sum2(Multiply(voice_v, In1), op_v(In2, In3)) -- the Sum2 form is served -- with In1 a row
    of +0 and the 6305 pairs in In2, In3, fed in blocks of 64 frames; bus: rows summed in pairs (its bus programs).  The gate
    makes the voice +-0, so every result survives the sum except a -0 beside a +0 voice term, which the expectation (float64
    reference on the oracle's voice) gives as +0 too."""
    import stream_input_cases as I
    a, b = pp.both_blocks()
    ops = pp.OPS + ("Minimum",) if bus else pp.OPS
    n = len(ops) // 2 if bus else len(ops)
    rows = [synth.time_ramp(0, len(a)), np.zeros(len(a), np.float32), a, b]
    got, plan = pp.stream_blocks(hip_lib, pp.stream_graph(ops, bus=bus), n, rows, I.STREAM_OPTIONS)
    s = plan["stream"]
    assert s["servable"] and s["kernel"] == "bank_stream_in_kernel" and s["input_slots"] == [0, 1, 2, 3], s
    assert s["bus_programs"] == (3 if bus else 0) and s["programs_per_voice"] == ([0] * 6 if bus else [1] * 5), s
    exp = pp.stream_expected(stream_voices[:len(ops)], rows[1], a, b, ops, bus=bus)
    msg = pp.first_diff("every op", f"stream control rows bus={bus}", a, b, got, exp)
    assert not msg, msg


@pytest.mark.parametrize("bus", [False, True], ids=["bank_stream_prog_kernel", "bank_stream_bus_kernel"])
@pytest.mark.parametrize("op", pp.OPS)
def test_stream_slot_0_programs(hip_lib, oracle_lib, op, bus):
    """The two interpreters without control rows read slot 0 only, so the signal is the voices' own time row: row v =
    Sum2(Multiply(voice_v, C(+0)), op(In0, C(H[v]))), 46 voices of 128 partials; bus: summed in pairs.  The row is a ramp, then
    H and 512 random patterns; the voice comes from the oracle on the same row."""
    import stream_input_cases as I
    consts = pp.H[:46]
    x = np.concatenate([synth.time_ramp(0, 81), pp.signal_row()])
    with Renderer(oracle_lib) as o:
        synth.install(o, pp.voices_tree(46, 128))
        voice = o.fill_buffer(46, 0, len(x), [x])
    got, plan = pp.stream_blocks(hip_lib, pp.stream_slot0_graph(op, consts, bus=bus), 23 if bus else 46, [x], I.STREAM_OPTIONS)
    s = plan["stream"]
    assert s["servable"] and s["input_slots"] == [0] and s["kernel"] == ("bank_stream_bus_kernel" if bus else "bank_stream_prog_kernel"), s
    exp = pp.stream_slot0_expected(voice, op, consts, x, bus=bus)
    msg = pp.first_diff(op, f"stream slot 0 bus={bus}", x, 0, got, exp)
    assert not msg, msg


# ---- the interpreters of feedback plans: stage_tile_kernel, stage_sweep_kernel -----------------------------------------------------
@pytest.fixture(scope="module")
def loop_rows_expected():
    """{sweep: row 1 of prim_pairs.loop_graph from the loop alone}, read-only."""
    out = {sweep: pp.loop_expected(sweep, pp.loop_rows(len(pp.both_blocks()[0]))) for sweep in (False, True)}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("op", pp.OPS)
@pytest.mark.parametrize("sweep", [False, True], ids=["stage_tile_kernel", "stage_sweep_kernel"])
def test_two_signals_beside_a_loop(hip_lib, reference_rows, loop_rows_expected, sweep, op):
    """SS on stage_tile_kernel (FR_LOOP_TILES=1, FR_STAGE_JIT=0, a loop of stride 3) and on stage_sweep_kernel (FR_LOOP_DYN=1,
    W = 7): op(In0, In1) on both blocks is a program of the feedback plan's one strided launch, beside a loop that it never
    meets (prim_pairs.loop_graph; the form is asserted from fr_plan_json).  Row 0 is the pair's reference, row 1 the loop's alone."""
    a, b = pp.both_blocks()
    for semantics in semantics_of(op):
        got = pp.render_beside_loop(hip_lib, op, sweep, semantics)
        msg = pp.first_diff(op, f"SS {semantics} beside a loop, sweep={sweep}", a, b, got[0], reference_rows[semantics][pp.OPS.index(op)])
        assert not msg, msg
        msg = pp.first_diff("the loop", f"beside {op}, sweep={sweep}", 0, 0, got[1], loop_rows_expected[sweep])
        assert not msg, msg


@pytest.mark.parametrize("semantics", SEMANTICS)
def test_hostile_amounts_in_a_sweep(hip_lib, semantics):
    """stage_sweep_kernel's Delays by a signal amount over a hostile amount row, every frame against the dense forward reference
    (prim_pairs.sweep_dyn_graph).  S_STEP_DYN and S_READ_INPUT_DYN get the row as it is: negative, NaN, +-inf, 2^64, fractional.
    S_READ_DYN of the loop's ring gets negative, -inf, -0, subnormal, fractional and NaN amounts (NaN: where reference and Sparkle
    part); +inf and 2^64 cannot reach a ring's read, whose ring needs a finite bound.  tests/loop_dyn_cases.py keeps every amount
    in [lo, hi] of its proof -- its hostile call feeds the LFO, which clamps --: none of these amounts occurs there."""
    got, exp = pp.sweep_dyn_rows(hip_lib, semantics)
    msg = pp.first_diff("Delay by a hostile amount", f"sweep {semantics}", 0, 0, got, exp)
    assert not msg, msg


# ---- block streaming's loop programs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", SEMANTICS)
def test_stream_loop_programs(hip_lib, reference_rows, semantics):
    """bank_stream_loops_kernel, stream_run_loop_program: row v = Sum2(Multiply(Multiply(x_v, x_v), In1), op_v(In2, In3)), x_v the
    voice through a comb of 5 frames, In1 a row of -0, the 6305 pairs in In2, In3, fed in blocks of 64 frames.  The op is in the
    loop's program (one loop program per voice, asserted); the loop's square times -0 is -0, and Sum2(-0, r) is r for every r:
    the rows are the pair's reference bit for bit."""
    import stream_loop_cases as SL
    a, b = pp.both_blocks()
    got, plan = pp.stream_blocks(hip_lib, pp.stream_loop_graph(), len(pp.OPS), pp.stream_loop_rows(), dict(SL.INPUTS, **SL.IDLE), semantics)
    pp.assert_loop_programs(plan["stream"], len(pp.OPS))
    msg = pp.first_diff("every op", f"stream loop programs {semantics}", a, b, got, reference_rows[semantics])
    assert not msg, msg
