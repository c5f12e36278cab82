"""The operand-pair matrix of the five arithmetic primitives (Sum2, Multiply, Divide, Modulo, Minimum), a plain float64
reference for them, the bit-for-bit comparison, and the graphs that carry a pair to each evaluator in each operand form
(plain data and graph recipes: importable without a GPU).  tests/test_prim_pairs.py runs the reference against both oracles
and every form through the engine's own host code on the host-logic simulator.

Operands.  H: 23 magnitudes with both signs and one NaN, 47 values -- zeros, the smallest and the largest subnormal,
FLT_MIN, values around 1, 2^24 and 2^24 + 1 as an f32 (which is 2^24 again: 45 distinct values), 2^32, huge values, FLT_MAX,
infinity.  The pair block is H x H (A = repeat(H, 47), B = tile(H, 47): 2209 frames); the random block is 4096 seeded pairs of uniformly random 32-bit
patterns (every exponent combination for the rounding of a quotient and for fmod).

Reference.  `reference(op, a, b, semantics)` computes per pair in float64 and rounds once to f32:
    Sum2 / Multiply / Divide   the binary64 result of binary32 operands, rounded to binary32, is the correctly rounded binary32
                               result (53 >= 2 * 24 + 2: the second rounding cannot move it)
    Modulo                     r = fmod(a, b), exact in any format; r < 0 ? r + b : r with the sum in float64, rounded once
    Minimum                    (a < b or isnan(b)) ? a : b; "sparkle": a NaN `a` wins
It walks no graph and imports nothing from the oracle.  The comparison is bit for bit: NaN equals NaN, +0 differs from -0.

Forms.  SS op(In0, In1); SP / PS op(In0, C(c)) and op(C(c), In0) with c different from row to row (generated code gets it as a
parameter); SL / LS the same with ONE constant shared by everything that shares code (generated code bakes it as a literal
where its rules allow); CC op(C(a), C(b)) (the host's constant folder).  No sample of any row is left out of a comparison."""
import numpy as np

from libfriendship_amd import synth

OPS = ("Sum2", "Multiply", "Divide", "Modulo", "Minimum")
KIND = {"Sum2": synth.K_SUM2, "Multiply": synth.K_MUL, "Divide": synth.K_DIV, "Modulo": synth.K_MOD, "Minimum": synth.K_MIN}

_MAGNITUDES = np.array([0.0, 1e-45, 3e-39, 1.1754942e-38, 1.17549435e-38, 1e-30, 0.1, 0.5, 0.75, 1.0, 1.0000001, 1.5, 2.0, 3.0, 7.25,
                        16777216.0, 16777217.0, 4294967296.0, 1e20, 1e30, 1.7014118e38, 3.4028235e38, np.inf], np.float32)
H = np.concatenate([np.stack([_MAGNITUDES, -_MAGNITUDES], axis=1).ravel(), np.array([np.nan], np.float32)]).astype(np.float32)
N_H = len(H)                      # 47
N_PAIRS = N_H * N_H               # 2209
N_RANDOM = 4096
RANDOM_SEED = 0x5EED0700

# Literal constants: generated stage programs bake +-0, +-1, +-0.5, +-2 (stagejit.cpp literal_worthy).
STAGE_LITERALS = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0], np.float32)


def pair_block():
    """(A, B): every pair of H, 2209 frames."""
    return np.repeat(H, N_H).astype(np.float32), np.tile(H, N_H).astype(np.float32)


def random_block(n=N_RANDOM, seed=RANDOM_SEED):
    """(A, B): n pairs of uniformly random 32-bit patterns (SplitMix64, seeded)."""
    z = synth.splitmix64(seed, n)
    return ((z >> np.uint64(32)).astype(np.uint32).view(np.float32).copy(), (z & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32).copy())


def both_blocks():
    """(A, B): the pair block followed by the random block, 6305 frames."""
    (a0, b0), (a1, b1) = pair_block(), random_block()
    return np.concatenate([a0, a1]), np.concatenate([b0, b1])


def signal_row():
    """The input of the one-signal forms: H, then the first 512 values of the random block's A (559 frames)."""
    return np.concatenate([H, random_block()[0][:512]])


# ---- the reference ------------------------------------------------------------------------------------------------------
def reference(op, a, b, semantics="reference"):
    """op(a, b) elementwise: float64 arithmetic on the f32 operands, rounded once to f32 (see the module's docstring)."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32))
    with np.errstate(all="ignore"):
        x, y = a.astype(np.float64), b.astype(np.float64)      # (exact; a signalling NaN of the random block raises "invalid")
        if op == "Sum2":
            return (x + y).astype(np.float32)
        if op == "Multiply":
            return (x * y).astype(np.float32)
        if op == "Divide":
            return (x / y).astype(np.float32)
        if op == "Modulo":
            r = np.fmod(x, y)
            return np.where(r < 0.0, r + y, r).astype(np.float32)
        if op == "Minimum":
            r = np.where((x < y) | np.isnan(y), a, b)
            if semantics == "sparkle":
                r = np.where(np.isnan(x), a, r)
            return r.astype(np.float32)
    raise KeyError(op)


# ---- the comparison -----------------------------------------------------------------------------------------------------
def differing(got, exp):
    """Boolean mask of the samples that differ bit for bit (NaN equals NaN; +0 differs from -0)."""
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    return ~((got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp)))


def first_diff(op, form, a, b, got, exp):
    """'' when got == exp bit for bit, else the op, the form, the operands and the bits of the first sample that differs.
    a, b: the operands, broadcastable to got's shape."""
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    bad = differing(got, exp)
    if not bad.any():
        return ""
    a, b = np.broadcast_to(np.asarray(a, np.float32), got.shape), np.broadcast_to(np.asarray(b, np.float32), got.shape)
    i = tuple(np.argwhere(bad)[0])
    bits = lambda v: f"{v!r} ({int(np.float32(v).view(np.uint32)):#010x})"
    return (f"{op} {form}: {int(bad.sum())} of {got.size} samples differ, first at {i}: a = {bits(a[i])}, b = {bits(b[i])}: "
            f"got {bits(got[i])}, expected {bits(exp[i])}")


# ---- graphs: one output row per (op, form, constant) ----------------------------------------------------------------------
def _rows(g, handles):
    handles = np.asarray(handles, np.uint32).ravel()
    g.edge(handles, 0, 0, np.arange(len(handles), dtype=np.uint32))
    return g.finish(len(handles))


def _operands(form, x, c):
    """(a, b) of a one-signal form: the signal x on the left (SP, SL) or on the right (PS, LS)."""
    return (x, c) if form in ("SP", "SL") else (c, x)


def ss_graph(ops=OPS):
    """Row per op: op(In0, In1).  Returns (tree, [(op, 'SS')])."""
    g = synth.GraphArrays()
    rows = [g.binop(KIND[op], synth.IN(0), synth.IN(1), 1)[0] for op in ops]
    return _rows(g, rows), [(op, "SS") for op in ops]


def sp_graph(ops=OPS, consts=H, forms=("SP", "PS")):
    """Rows op(In0, C(c)) (SP) and op(C(c), In0) (PS) for every c of `consts`.  Returns (tree, [(op, form, c)]) in row order."""
    g = synth.GraphArrays()
    rows, meta = [], []
    consts = np.asarray(consts, np.float32)
    for op in ops:
        for form in forms:
            a, b = _operands(form, synth.IN(0), synth.C(consts))
            rows.append(g.binop(KIND[op], a, b, len(consts)))
            meta += [(op, form, c) for c in consts]
    return _rows(g, np.concatenate(rows)), meta


def sl_graph(literal, ops=OPS):
    """The ten rows of one literal: op(In0, C(L)) (SL) and op(C(L), In0) (LS) per op -- every constant of the graph is L, so
    whatever shares generated code agrees on it.  Returns (tree, [(op, form, L)])."""
    tree, meta = sp_graph(ops, np.array([literal], np.float32))
    return tree, [(op, {"SP": "SL", "PS": "LS"}[form], c) for op, form, c in meta]


def cc_graph(op, a, b):
    """Row per pair: op(C(a_i), C(b_i)) -- the host folds each to a constant at lowering (graph.cpp FlatGraph::make)."""
    g = synth.GraphArrays()
    return _rows(g, g.binop(KIND[op], synth.C(a), synth.C(b), len(a)))


def one_signal_expected(meta, x, semantics="reference"):
    """[len(meta), len(x)]: the reference of every row of sp_graph / sl_graph on the input row x; and the operands, for
    first_diff."""
    exp = np.empty((len(meta), len(x)), np.float32)
    A = np.empty_like(exp)
    B = np.empty_like(exp)
    for r, (op, form, c) in enumerate(meta):
        A[r], B[r] = _operands(form, x, np.float32(c))
        exp[r] = reference(op, A[r], B[r], semantics)
    return exp, A, B


# ---- generated voice leaves: a voice is a balanced sum of P leaves of one shape ------------------------------------------------
# P IDENTICAL leaves op(., .) are interned at lowering (one node) and plan as a stage program, so every leaf here is the
# operation times its own exact power of two, 2^-(k + 1): leaves of one shape that differ in one parameter, which is what the
# matcher takes for a compiled voice.  The expectation multiplies and sums with the float64 reference in the tree's
# association; a one-ulp error of op(., .) is 1 to 1.875 ulp of the sum before its rounding, so it stays visible.
LEAF_LITERALS = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0, -2.0, 4.0, np.inf, np.nan, 1e-45], np.float32)
FMA_LITERALS = np.array([2.0, -4.0], np.float32)


def leaf_scales(P):
    return (2.0 ** -(1.0 + np.arange(P, dtype=np.float64))).astype(np.float32)


def leaf_graph(op, form, consts, P):
    """len(consts) voices (rows) of P leaves  2^-(k + 1) * body.  body: SS op(In0, In1); SP / SL op(In0, C(c_v)); PS / LS
    op(C(c_v), In0); form "FMA" (op ignored): Sum2(In0, Multiply(C(c_v), In1))."""
    consts = np.asarray(consts, np.float32).ravel()
    V = len(consts)
    g = synth.GraphArrays()
    c = synth.C(np.repeat(consts, P))
    if form == "SS":
        body = g.binop(KIND[op], synth.IN(0), synth.IN(1), V * P)
    elif form == "FMA":
        body = g.binop(synth.K_SUM2, synth.IN(0), g.binop(synth.K_MUL, c, synth.IN(1), V * P), V * P)
    else:
        a, b = _operands(form, synth.IN(0), c)
        body = g.binop(KIND[op], a, b, V * P)
    leaves = g.binop(synth.K_MUL, synth.C(np.tile(leaf_scales(P), V)), body, V * P)
    return _rows(g, synth.sum_tree(g, leaves.reshape(V, P)))


def tree_sum(leaves):
    """The balanced pairwise sum over the last axis (synth.sum_tree's association) with the reference's Sum2."""
    while leaves.shape[-1] > 1:
        leaves = reference("Sum2", leaves[..., 0::2], leaves[..., 1::2])
    return leaves[..., 0]


def leaf_expected(op, form, consts, P, x, y=None, semantics="reference"):
    """[len(consts), len(x)] and the operands (A, B) of op for first_diff."""
    consts = np.asarray(consts, np.float32).ravel()[:, None]
    x = np.asarray(x, np.float32)[None, :]
    if form == "SS":
        A, B = np.broadcast_arrays(x, np.asarray(y, np.float32)[None, :])
        r = reference(op, A, B, semantics)
    elif form == "FMA":
        A, B = np.broadcast_arrays(x, reference("Multiply", consts, np.asarray(y, np.float32)[None, :]))
        r = reference("Sum2", A, B)
    else:
        A, B = np.broadcast_arrays(*_operands(form, x, consts))
        r = reference(op, A, B, semantics)
    return tree_sum(reference("Multiply", leaf_scales(P)[None, None, :], r[..., None])), A, B


# ---- block streaming: a program per voice that reads the pair from control rows -------------------------------------------------
def _stream_voices(g, V, P, seed=0x5EED0700):
    p = synth.voice_params(V, P, seed, True, wrap=24)
    return synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P))


def voices_tree(V, P):
    """The voices alone, a row each: what the oracle is asked for."""
    g = synth.GraphArrays()
    return _rows(g, _stream_voices(g, V, P))


def stream_graph(ops=OPS, P=128, bus=False, product=False):
    """Row v = Sum2(Multiply(voice_v, In1), op_v(In2, In3)) (product: Multiply(voice_v, op_v(In2, In3))); bus: every two
    neighbouring rows summed into one."""
    g = synth.GraphArrays()
    V = len(ops)
    x = _stream_voices(g, V, P)
    r = np.concatenate([g.binop(KIND[op], synth.IN(2), synth.IN(3), 1) for op in ops])
    y = g.binop(synth.K_MUL, x, r, V) if product else g.binop(synth.K_SUM2, g.binop(synth.K_MUL, x, synth.IN(1), V), r, V)
    if bus:
        y = synth.sum_tree(g, y.reshape(V // 2, 2))
    return _rows(g, y)


def stream_expected(voice, gate, a, b, ops=OPS, bus=False, product=False, semantics="reference"):
    """voice: [len(ops), T], the oracle's rendering of voices_tree on the same time row; gate: the In1 row."""
    r = np.stack([reference(op, a, b, semantics) for op in ops])
    y = reference("Multiply", voice, r) if product else reference("Sum2", reference("Multiply", voice, gate[None, :]), r)
    return tree_sum(y.reshape(len(ops) // 2, 2, -1).transpose(0, 2, 1)) if bus else y


def stream_slot0_graph(op, consts, P=128, bus=False):
    """Programs that read slot 0 only (the kernels without control rows): row v = Sum2(Multiply(voice_v, C(+0)),
    op(In0, C(c_v))), the signal being the voices' own time row; bus: every two neighbouring rows summed into one."""
    consts = np.asarray(consts, np.float32).ravel()
    g = synth.GraphArrays()
    V = len(consts)
    x = _stream_voices(g, V, P)
    r = g.binop(KIND[op], synth.IN(0), synth.C(consts), V)
    y = g.binop(synth.K_SUM2, g.binop(synth.K_MUL, x, synth.C(np.zeros(V, np.float32)), V), r, V)
    if bus:
        y = synth.sum_tree(g, y.reshape(V // 2, 2))
    return _rows(g, y)


def stream_slot0_expected(voice, op, consts, x, bus=False, semantics="reference"):
    consts = np.asarray(consts, np.float32).ravel()[:, None]
    r = reference(op, x[None, :], consts, semantics)
    y = reference("Sum2", reference("Multiply", voice, np.float32(0.0)), r)
    return tree_sum(y.reshape(len(consts) // 2, 2, -1).transpose(0, 2, 1)) if bus else y


# ---- the interpreters that only feedback plans reach: the op beside a loop that never meets it -------------------------------------
# stage_tile_kernel and stage_sweep_kernel run every program of a feedback plan's strided launch, so row 0 = op(In0, In1) is a
# program of its own beside the loop's (row 1), in the same launch: no edge joins the two, row 0's expectation is the float64
# reference of the pair alone, row 1's the dense reference of the loop alone on its own finite rows.
LOOP_TILES = {"FR_LOOP_TILES": "1", "FR_STAGE_JIT": "0"}
LOOP_SWEEP = {"FR_LOOP_DYN": "1"}
LOOP_GAIN = 0.5


def loop_rows(n, seed=0x5EED0900):
    """The loop's own rows: finite noise (its input) and the frame ramp (the sweep's LFO)."""
    return [np.random.default_rng(seed).normal(size=n).astype(np.float32), np.arange(n, dtype=np.float32)]


def _loop_beside(g, sweep):
    """x = In2 + 0.5 * Delay(x, d): d = 3 frames (a stride of 3: tiled), or sweep: 8 + 6 * lfo(In3), proven >= 7 (W = 7)."""
    import loop_dyn_cases as LD
    x = g.node("Sum2")
    g.connect(("in", 2), x, 0)
    g.connect(g.op("Multiply", g.op("Delay", x, LD.amount(g, 8.0, 6.0, slot=3) if sweep else ("c", 3.0)), ("c", LOOP_GAIN)), x, 1)
    return x


def loop_graph(op, sweep=False):
    """Row 0 = op(In0, In1); row 1 = the loop on In2 (and In3)."""
    from stage_reference import Graph
    g = Graph()
    g.output(g.op(op, ("in", 0), ("in", 1)), 0)
    g.output(_loop_beside(g, sweep), 1)
    return g


def loop_alone(sweep=False):
    """The loop of loop_graph with no other row (input slots 0 and 1 unused): what its row is compared with."""
    from stage_reference import Graph
    g = Graph()
    g.output(_loop_beside(g, sweep), 0)
    return g


def loop_expected(sweep, rows):
    """Row 1 of loop_graph from the loop alone: the dense references of the feedback tests (stage_reference.DenseReference for
    the constant delay, loop_dyn_reference.DenseForward for the signal amount).  The pair's rows are not passed."""
    import loop_dyn_reference as ldr
    import stage_reference as sr
    n = len(rows[0])
    store = sr.InputStore()
    store.call(0, [np.zeros(n, np.float32), np.zeros(n, np.float32)] + list(rows))
    return (ldr.DenseForward if sweep else sr.DenseReference)(loop_alone(sweep))(store, 0, n)[0]


def render_beside_loop(lib, op, sweep, semantics):
    """op(In0, In1) on both blocks beside the loop: the two rows, after asserting from fr_plan_json that ONE launch of the form
    ran both programs (stage_tile_kernel: a +tile variant; stage_sweep_kernel)."""
    from libfriendship_amd.capi import Renderer
    a, b = both_blocks()
    g = loop_graph(op, sweep)
    with Renderer(lib, mode="staged", options=LOOP_SWEEP if sweep else LOOP_TILES, semantics=semantics) as r:
        g.install(r)
        got = r.fill_buffer(2, 0, len(a), [a, b] + loop_rows(len(a)))
        plan = r.plan()
    launches = plan["stage_launches"]
    assert plan["feedback"] and plan["pull_rows"] == 0 and not plan["stage_jit"] and len(launches) == 1 and launches[0]["programs"] == 2, (plan["pull_rows"], launches)
    if sweep:
        assert launches[0]["variant"] == "stage_sweep_kernel/feedback+sweep" and 1 <= plan["loop_dyn"]["frames"] <= 256, (launches, plan["loop_dyn"])
    else:
        kernel, form = launches[0]["variant"].split("/")
        assert kernel == "stage_kernel" and "tile" in form.split("+") and 1 <= plan["fused_stride"] <= 64 and plan["loop_tiles"]["frames"], (launches, plan["loop_tiles"])
    return got


# Delays by a HOSTILE amount in a sweep plan.  The loop's own Delay is the flanger's (a sweep needs its proof); behind it, all in
# stage_sweep_kernel: row 1 = Delay(C(2.5), In2) (S_STEP_DYN) and row 2 = Delay(In0, In2) (S_READ_INPUT_DYN) take the amount row
# as it is -- negative, NaN, +-inf, 2^64, fractional.  S_READ_DYN reads a ring (the loop's, from the next level), and a ring's
# size needs a finite upper bound of the amount: +inf and 2^64 cannot reach it in a staged plan.  Everything else does, on rows
# 3 to 5 (SWEEP_RING_AMOUNTS): Minimum(C(5), In2) passes the negative, -inf, -0, subnormal and fractional amounts (NaN, +inf and
# 2^64 become 5); Modulo(In2, C(8)) is NaN for the NaN and the +-inf entries, in both semantics; Minimum(In2, C(5)) is NaN for
# the NaN entries under Sparkle.  NaN is where the semantics part for a ring's read: the reference delays by 0 frames, Sparkle
# yields 0.
SWEEP_RING_AMOUNTS = (("Minimum", 5.0, True), ("Modulo", 8.0, False), ("Minimum", 5.0, False))     # (op, constant, constant on the left)


def sweep_ring_amounts(amt, semantics):
    """The amounts that reach S_READ_DYN on rows 3 to 5, by the float64 reference."""
    return [reference(op, np.float32(c), amt, semantics) if left else reference(op, amt, np.float32(c), semantics) for op, c, left in SWEEP_RING_AMOUNTS]


def hostile_amounts(n):
    import stage_variants as sv
    amounts = (np.arange(n) % 9).astype(np.float32) + np.float32(0.25) * (np.arange(n) % 4).astype(np.float32)
    amounts[1::3] = np.resize(sv.HOSTILE_AMOUNTS, len(amounts[1::3]))
    return amounts


def sweep_dyn_graph():
    import loop_dyn_cases as LD
    from stage_reference import Graph
    g = Graph()
    x = g.node("Sum2")
    g.connect(("in", 0), x, 0)
    g.connect(g.op("Multiply", g.op("Delay", x, LD.amount(g, 8.0, 6.0, slot=1)), ("c", LOOP_GAIN)), x, 1)
    g.output(x, 0)
    g.output(g.op("Delay", ("c", 2.5), ("in", 2)), 1)
    g.output(g.op("Delay", ("in", 0), ("in", 2)), 2)
    for k, (op, c, left) in enumerate(SWEEP_RING_AMOUNTS):
        g.output(g.op("Delay", x, g.op(op, ("c", c), ("in", 2)) if left else g.op(op, ("in", 2), ("c", c))), 3 + k)
    return g


def sweep_dyn_rows(lib, semantics, n=1500):
    """sweep_dyn_graph on `lib` over n frames, after asserting from fr_plan_json that both levels ran as sweeps: the rows and the
    dense forward reference's."""
    import loop_dyn_reference as ldr
    import stage_reference as sr
    from libfriendship_amd.capi import Renderer
    g = sweep_dyn_graph()
    rows = loop_rows(n) + [hostile_amounts(n)]
    amt = rows[2]
    assert np.isnan(amt).any() and (amt == np.inf).any() and (amt == -np.inf).any() and (amt < 0).any() and (amt == 2.0 ** 64).any()
    assert (np.isfinite(amt) & (amt != np.floor(amt))).any()
    ring = sweep_ring_amounts(amt, semantics)                            # what S_READ_DYN gets: no +inf, no 2^64, everything else
    assert (ring[0] < 0).any() and (ring[0] == -np.inf).any() and (np.isfinite(ring[0]) & (ring[0] != np.floor(ring[0]))).any()
    assert np.isnan(ring[1]).sum() >= n // 20 and np.isnan(ring[2]).any() == (semantics == "sparkle")
    assert not any(((a == np.inf) | (a >= 2.0 ** 64)).any() for a in ring)
    n_out = 3 + len(ring)
    with Renderer(lib, mode="staged", options=LOOP_SWEEP, semantics=semantics) as r:
        g.install(r)
        got = r.fill_buffer(n_out, 0, n, rows)
        plan = r.plan()
    variants = [l["variant"] for l in plan["stage_launches"]]
    assert plan["pull_rows"] == 0 and variants == ["stage_sweep_kernel/feedback+sweep"] * 2 and plan["loop_dyn"]["frames"] == 7, (plan["pull_rows"], variants)
    store = sr.InputStore()
    store.call(0, rows)
    exp = ldr.DenseForward(g, semantics)(store, 0, n)
    assert all((exp[r] != 0).sum() > n // 2 for r in range(n_out))      # (every Delay yields more than its zeros)
    return got, exp


# Block streaming's loop programs.  A streamed program is a voice's, and a loop program is the ONE program that holds the loop, so
# the op sits in the loop's program: row v = Sum2(Multiply(Multiply(x_v, x_v), In1), op_v(In2, In3)) with x_v = voice_v + 0.5 *
# Delay(x_v, 5).  The op does not enter the loop.  The loop enters the row as its square -- finite, never negative -- times In1,
# a row of -0: that product is -0 on every frame whatever x is, and Sum2(-0, r) is r for EVERY r, -0 and +0 included (NaN stays
# NaN).  So the expectation is the float64 reference of the pair alone; no voice and no loop value is needed for it.
STREAM_LOOP_DELAY = 5


def stream_loop_graph(ops=OPS, P=128):
    g = synth.GraphArrays()
    V = len(ops)
    dl = g.nodes(synth.K_DELAY, V)
    g.const(dl, np.float32(STREAM_LOOP_DELAY), 1)
    x = g.binop(synth.K_SUM2, _stream_voices(g, V, P), g.binop(synth.K_MUL, dl, synth.C(np.float32(LOOP_GAIN)), V), V)
    g.edge(x, dl, 0, 0)
    r = np.concatenate([g.binop(KIND[op], synth.IN(2), synth.IN(3), 1) for op in ops])
    return _rows(g, g.binop(synth.K_SUM2, g.binop(synth.K_MUL, g.binop(synth.K_MUL, x, x, V), synth.IN(1), V), r, V))


def stream_loop_rows():
    """[time ramp, the gate of -0, In2, In3] over both blocks."""
    a, b = both_blocks()
    return [synth.time_ramp(0, len(a)), np.full(len(a), -0.0, np.float32), a, b]


def assert_loop_programs(s, n):
    """fr_plan_json["stream"]: servable by the loops kernel, a loop program (stride STREAM_LOOP_DELAY) per voice and no other."""
    assert s["servable"] and s["kernel"] == "bank_stream_loops_kernel", s
    assert s["loop_programs"] == [STREAM_LOOP_DELAY] * n and s["programs_per_voice"] == [1] * n and s["bus_programs"] == 0, s


# ---- running a recipe on a library (the simulator's or the device's) and asserting the evaluator from the plan ---------------------
SEMANTICS = ("reference", "sparkle")
EVALUATORS = {"pull": ("pull", {}), "stage_kernel": ("staged", {"FR_STAGE_JIT": "0"}), "stage_jit": ("staged", {"FR_STAGE_JIT": "force"})}
CC_FRAMES = 3
STREAM_BLOCK = 64


def semantics_of(op):
    return SEMANTICS if op == "Minimum" else SEMANTICS[:1]


def reference_rows():
    """{semantics: [5, 6305]}: the float64 reference of every op on both blocks, read-only."""
    a, b = both_blocks()
    out = {s: np.stack([reference(op, a, b, s) for op in OPS]) for s in SEMANTICS}
    for v in out.values():
        v.setflags(write=False)
    return out


def assert_evaluator(plan, ev, n_rows):
    variants = [l["variant"] for l in plan["stage_launches"]]
    if ev == "pull":
        assert plan["pull_rows"] == n_rows and not variants and not plan["banks"], (plan["pull_rows"], variants, plan["banks"])
        return
    assert plan["pull_rows"] == 0 and not plan["banks"] and variants, (plan["pull_rows"], plan["banks"], variants)
    if ev == "stage_jit":
        assert plan["stage_jit"] and all(v.split("/")[0] != "stage_kernel" for v in variants), (plan["stage_jit"], variants)
    else:
        assert not plan["stage_jit"] and all(v.split("/")[0] == "stage_kernel" for v in variants), (plan["stage_jit"], variants)


def render(lib, tree, n_rows, rows, ev, semantics, check_plan=None):
    """check_plan(plan): what else the caller asserts from fr_plan_json."""
    from libfriendship_amd.capi import Renderer
    mode, options = EVALUATORS[ev]
    with Renderer(lib, mode=mode, options=options, semantics=semantics) as r:
        synth.install(r, tree)
        got = r.fill_buffer(n_rows, 0, len(rows[0]), rows)
        plan = r.plan()
        assert_evaluator(plan, ev, n_rows)
        if check_plan:
            check_plan(plan)
        return got


def render_leaves(lib, tree, n_rows, rows, P, k, options=None, semantics="reference", compiled=True):
    """A leaf_graph in mode "auto".  compiled: every voice must have run as a hipRTC-compiled bank of P leaves with k varying
    parameters per leaf (the simulator has no run-time compiler: there the voices run as stage programs)."""
    from libfriendship_amd.capi import Renderer
    with Renderer(lib, options=options, semantics=semantics) as r:
        synth.install(r, tree)
        got = r.fill_buffer(n_rows, 0, len(rows[0]), rows)
        plan = r.plan()
    assert plan["pull_rows"] == 0, plan["pull_rows"]
    if compiled:
        banks = plan["banks"]
        assert banks and sum(b["voices"] for b in banks) == n_rows and not plan["stage_launches"], (banks, plan["stage_launches"])
        assert all(b["jit"] and b["partials"] == P and b["leaf_params"] == k for b in banks), banks
        assert all(l["kernel"] in ("jit_bank", "jit_bank_multi") for l in plan["bank_launches"]), plan["bank_launches"]
    return got


def stream_blocks(lib, tree, n_rows, rows, options, semantics="reference"):
    """The rows fed block by block (STREAM_BLOCK frames) through fr_stream_block_rows from frame 0: the output and the plan."""
    from libfriendship_amd.capi import Renderer
    N = len(rows[0])
    with Renderer(lib, semantics=semantics, options=options) as s:
        synth.install(s, tree)
        s.stream_begin(n_rows)
        got = np.concatenate([s.stream_block_rows(i, [r[i:i + STREAM_BLOCK] for r in rows], n_times=min(STREAM_BLOCK, N - i))
                              for i in range(0, N, STREAM_BLOCK)], axis=1)
        plan = s.plan()
        s.stream_end()
    return got, plan
