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


def render(lib, tree, n_rows, rows, ev, semantics):
    from libfriendship_amd.capi import Renderer
    mode, options = EVALUATORS[ev]
    with Renderer(lib, mode=mode, options=options, semantics=semantics) as r:
        synth.install(r, tree)
        got = r.fill_buffer(n_rows, 0, len(rows[0]), rows)
        assert_evaluator(r.plan(), ev, n_rows)
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
